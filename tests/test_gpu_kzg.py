"""Polynomial evaluation, Ruffini division and KZG openings on the device (lw_poly_*, lw_kzg_*) against the values the
reference's PLONK tests hard-code (test_round_4 / test_round_5, tests/golden/plonk_round_4_5.json) and against Python
big-integer Horner / Ruffini and the oracle MSM.

Every division is checked byte for byte in the stored (Montgomery) form: with R = 2^256, the stored values A_i = a_i R and
X = x R satisfy the same recurrence C_i = A_i + (X / R) C_{i+1} mod p, so a Python Ruffini over the raw stored integers
with multiplier X R^-1 gives the raw stored quotient.

The kernels' schedule (lambda_elliptic_curves_amd/csrc/poly.hip): 8 consecutive coefficients per thread, tiles of
256 x 8 = 2048 per block, and the carry scan gives each of its 256 threads ceil(tiles / 256) tiles — so the boundaries are
n = 8, 2048, and 256 * 2048 = 2^19 (one more tile per scan thread), each straddled below."""
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from oracle import bigint_def as D
from oracle import oracle as O
from tests import plonk_kat_round45 as K
from tests import util

pytestmark = pytest.mark.gpu
H = lambda s: int(s, 16)
MODULI = {"stark252": D.P_STARK252, "fr381": D.P_FR381}
BOUNDARY_SIZES = [0, 1, 2, 3, 7, 8, 9, 2047, 2048, 2049, 4097, (1 << 19) - 1, 1 << 19, (1 << 19) + 1]


def to_ints(a):
    a = np.ascontiguousarray(a, dtype=np.uint64).reshape(-1, 4)
    b = a.astype(">u8").tobytes()
    return [int.from_bytes(b[32 * i:32 * i + 32], "big") for i in range(a.shape[0])]


def to_arr(vals):
    if not len(vals):
        return np.zeros((0, 4), np.uint64)
    b = b"".join(int(v).to_bytes(32, "big") for v in vals)
    return np.frombuffer(b, dtype=">u8").astype(np.uint64).reshape(-1, 4)


def rinv(p):
    return pow(1 << 256, -1, p)


def mont(vals, p):
    return to_arr([v * (1 << 256) % p for v in vals])


def unmont(a, p):
    ri = rinv(p)
    return [v * ri % p for v in to_ints(a)]


def fld(name):
    from lambda_elliptic_curves_amd import fft
    return {"stark252": fft.Stark252PrimeField, "fr381": fft.FrField}[name]


def special_points(p, coeffs_raw, rng):
    """stored x values: 0, 1, -1, a random one, and a root of the (adjusted) polynomial, returned with the adjusted
    coefficients"""
    one = (1 << 256) % p
    xs = [0, one, (p - one) % p, int(rng.integers(1, 1 << 62)) * 0x9e3779b97f4a7c15 % p]
    root = int(rng.integers(2, 1 << 62)) % p
    a = list(coeffs_raw)
    if len(a) >= 2:   # make the stored root a root of the polynomial: A_0 = -sum_{i >= 1} A_i r^i with r = root R^-1
        r = root * rinv(p) % p
        a[0] = (-K.horner([0] + a[1:], r, p)) % p
        xs.append(root)
    return xs, a


@pytest.mark.parametrize("name", ["stark252", "fr381"])
def test_ruffini_division_matches_python(name):
    from lambda_elliptic_curves_amd import poly
    p, F = MODULI[name], fld(name)
    rng = np.random.default_rng(11)
    sizes = BOUNDARY_SIZES + [int(v) for v in rng.integers(10, 20000, 3)]
    for n in sizes:
        a = to_ints(util.rand_elems(name, n, 100 + n))
        xs, a = special_points(p, a, rng)
        root = xs[4] if len(xs) == 5 else None
        if n > 5000:
            xs = xs[-1:]   # the large sizes: one point (the root)
        for X in xs:
            q_want, rem_want = K.ruffini(a, X * rinv(p) % p, p)
            q, rem = poly.ruffini_division(F, to_arr(a), to_arr([X])[0])
            assert to_ints(q) == q_want, (name, n, X)
            assert to_ints(rem.reshape(1, 4))[0] == rem_want, (name, n, X)
            if X == root:
                assert rem_want == 0


@pytest.mark.parametrize("name", ["stark252", "fr381"])
def test_ruffini_division_2_20_device(name):
    import torch
    from lambda_elliptic_curves_amd import poly
    p, F = MODULI[name], fld(name)
    n = 1 << 20
    arr = util.rand_elems(name, n, 5)
    a = to_ints(arr)
    X = to_ints(util.rand_elems(name, 1, 6))[0]
    q_want, rem_want = K.ruffini(a, X * rinv(p) % p, p)
    t_a = torch.from_numpy(arr.view(np.int64)).cuda()
    t_q = torch.empty((n - 1, 4), dtype=torch.int64, device="cuda")
    rem = poly.ruffini_division_device(F, t_a, n, to_arr([X])[0], t_q)
    torch.cuda.synchronize()
    assert to_ints(rem.reshape(1, 4))[0] == rem_want
    assert to_ints(t_q.cpu().numpy().view(np.uint64)) == q_want
    # without the remainder: no synchronisation inside, the same quotient once the stream has run
    t_q2 = torch.zeros_like(t_q)
    assert poly.ruffini_division_device(F, t_a, n, to_arr([X])[0], t_q2, remainder=False) is None
    torch.cuda.synchronize()
    assert torch.equal(t_q, t_q2)


@pytest.mark.parametrize("name", ["stark252", "fr381"])
def test_evaluate_matches_horner(name):
    import torch
    from lambda_elliptic_curves_amd import poly
    p, F = MODULI[name], fld(name)
    lens = [0, 1, 7, 2049, 5000, 3, 4096]
    polys = [util.rand_elems(name, n, 40 + i) for i, n in enumerate(lens)]
    pts = util.rand_elems(name, 6, 77)          # 6 points: more than one launch's worth (4)
    pts[0] = 0
    xe = [v * rinv(p) % p for v in to_ints(pts)]
    want = [[K.horner(to_ints(a), x, p) for x in xe] for a in polys]
    got = poly.evaluate(F, polys, pts)
    assert got.shape == (len(lens), 6, 4)
    assert [to_ints(row) for row in got] == want
    t_polys = [torch.from_numpy(a.view(np.int64)).cuda() if len(a) else torch.zeros((1, 4), dtype=torch.int64, device="cuda")
               for a in polys]
    got_d = poly.evaluate_device(F, t_polys, lens, pts)
    assert np.array_equal(got_d, got)


def _proof_aff(oid, pt):
    return O.point_to_affine_ints(oid, pt)


def _canon_case(r, n, seed):
    rng = np.random.default_rng(seed)
    a = [int(v) % r for v in rng.integers(0, 1 << 63, size=(n,), dtype=np.uint64)]
    a = [(v << 190 | int(rng.integers(0, 1 << 62))) % r for v in a]
    x = int(rng.integers(1, 1 << 62)) * 0x1234567 % r
    return a, x


@pytest.mark.parametrize("name,r", [("bls12_381_g1", D.P_FR381), ("bn254_g1", D.P_FR254)])
def test_open_matches_oracle_msm_of_python_quotient(name, r):
    from lambda_elliptic_curves_amd import kzg, msm
    crv, oid = util.curve_pairs()[name]
    top = 1 << 16
    _, points = util.msm_case(oid, top, 31, threads=util.host_threads())
    srs = msm.Srs(crv, points)
    try:
        for n in (1 << 12, (1 << 14) + 3, 1 << 16):
            a, x = _canon_case(r, n, n)
            q, ev = K.ruffini(a, x, r)
            proof, got_ev = kzg.open(srs, mont(a, r), mont([x], r)[0])
            assert unmont(got_ev.reshape(1, 4), r)[0] == ev
            want = O.parallel_msm_with(oid, O.ints_to_array(q, 4), points[:n - 1], 12, util.host_threads())
            assert _proof_aff(oid, proof) == _proof_aff(oid, want), (name, n)
    finally:
        srs.close()


def test_open_small_lengths_and_srs_too_short():
    from lambda_elliptic_curves_amd import errors, kzg, msm
    crv, oid = util.curve_pairs()["bls12_381_g1"]
    r = D.P_FR381
    _, points = util.msm_case(oid, 16, 9)
    srs = msm.Srs(crv, points)
    try:
        x = mont([5], r)[0]
        for n in (0, 1):   # the neutral point; p(x) = 0 / a_0
            a = mont([7] * n, r)
            proof, ev = kzg.open(srs, a, x)
            assert _proof_aff(oid, proof) is None
            assert unmont(ev.reshape(1, 4), r)[0] == (7 if n else 0)
        a, xi = _canon_case(r, 17, 1)            # quotient of 16 = the SRS length: fine
        q, _ = K.ruffini(a, xi, r)
        proof, _ = kzg.open(srs, mont(a, r), mont([xi], r)[0])
        assert _proof_aff(oid, proof) == _proof_aff(oid, O.msm(oid, O.ints_to_array(q, 4), points))
        with pytest.raises(errors.LengthMismatch):   # quotient of 17 > 16 points
            kzg.open(srs, mont(_canon_case(r, 18, 2)[0], r), x)
        with pytest.raises(errors.LengthMismatch):
            kzg.open_batch(srs, [mont([1] * 3, r), mont([1] * 18, r)], x, x)
    finally:
        srs.close()


def test_open_through_a_folded_srs(monkeypatch):
    from lambda_elliptic_curves_amd import kzg, msm
    crv, oid = util.curve_pairs()["bls12_381_g1"]
    r = D.P_FR381
    _, points = util.msm_case(oid, 3000, 55)
    monkeypatch.setenv("LW_HIP_SRS_FOLD_MIN", "0")
    srs = msm.Srs(crv, points)
    try:
        for n in (3001, 1500):   # above and below the quarter that switches back to the plain schedule
            a, x = _canon_case(r, n, 70 + n)
            q, _ = K.ruffini(a, x, r)
            proof, _ = kzg.open(srs, mont(a, r), mont([x], r)[0])
            want = O.parallel_msm_with(oid, O.ints_to_array(q, 4), points[:n - 1], 8, util.host_threads())
            assert _proof_aff(oid, proof) == _proof_aff(oid, want), n
    finally:
        srs.close()


def test_open_batch_equals_open_of_folded_polynomial():
    import torch
    from lambda_elliptic_curves_amd import kzg, msm
    crv, oid = util.curve_pairs()["bls12_381_g1"]
    r = D.P_FR381
    _, points = util.msm_case(oid, 6000, 8)
    srs = msm.Srs(crv, points)
    rng = np.random.default_rng(12)
    try:
        x = to_ints(util.rand_elems("fr381", 1, 3))[0]
        for k in range(1, 10):
            lens = [int(v) for v in rng.integers(0, 6000, k)]
            lens[k // 2] = 5001
            polys = [util.rand_elems("fr381", n, 1000 * k + i) for i, n in enumerate(lens)]
            for U in (0, (1 << 256) % r, to_ints(util.rand_elems("fr381", 1, k))[0]):
                ue = U * rinv(r) % r
                folded = K.fold([to_ints(p) for p in polys], ue)   # stored form: u^k acts through U R^-1
                proof, evs = kzg.open_batch(srs, polys, to_arr([x])[0], to_arr([U])[0])
                want, _ = kzg.open(srs, to_arr(folded), to_arr([x])[0])
                assert _proof_aff(oid, proof) == _proof_aff(oid, want), (k, U)
                xe = x * rinv(r) % r
                assert to_ints(evs) == [K.horner(to_ints(p), xe, r) for p in polys], (k, U)
            if k in (1, 7):   # the device form
                t = [torch.from_numpy(p.view(np.int64)).cuda() if len(p) else torch.zeros((1, 4), dtype=torch.int64, device="cuda")
                     for p in polys]
                proof_d, evs_d = kzg.open_batch_device(srs, t, lens, to_arr([x])[0], to_arr([U])[0])
                assert _proof_aff(oid, proof_d) == _proof_aff(oid, proof) and np.array_equal(evs_d, evs)
    finally:
        srs.close()


def test_large_open_equals_srs_msm_of_device_quotient():
    import torch
    from lambda_elliptic_curves_amd import fft, kzg, msm, poly
    crv, oid = util.curve_pairs()["bls12_381_g1"]
    n = 1 << 22
    _, points = util.msm_case(oid, n, 4, threads=util.host_threads())
    srs = msm.Srs(crv, points)
    try:
        arr = util.rand_elems("fr381", n, 21)
        x = util.rand_elems("fr381", 1, 22)[0]
        t_a = torch.from_numpy(arr.view(np.int64)).cuda()
        t_q = torch.empty((n - 1, 4), dtype=torch.int64, device="cuda")
        rem = poly.ruffini_division_device(fft.FrField, t_a, n, x, t_q)
        want = srs.msm_fr_device(t_q, n - 1)
        proof, ev = kzg.open_device(srs, t_a, n, x)
        assert np.array_equal(ev, rem)
        assert _proof_aff(oid, proof) == _proof_aff(oid, want)
    finally:
        srs.close()


def _evaluator(device):
    """round 4's evaluate through lw_poly_evaluate (host buffers) or lw_poly_evaluate_device"""
    from lambda_elliptic_curves_amd import fft, poly
    r = D.P_FR381

    def ev(ps, xs):
        arrs = [mont(p, r) for p in ps]
        if device:
            import torch
            t = [torch.from_numpy(a.view(np.int64)).cuda() for a in arrs]
            got = poly.evaluate_device(fft.FrField, t, [len(p) for p in ps], mont(xs, r))
        else:
            got = poly.evaluate(fft.FrField, arrs, mont(xs, r))
        return [unmont(row, r) for row in got]
    return ev


@pytest.mark.parametrize("device", [False, True])
def test_hip_path_reproduces_reference_round_4_and_5(device):
    import torch
    from lambda_elliptic_curves_amd import kzg, msm
    oid = O.C_BLS12_381_G1
    r = D.P_FR381
    g = K.golden()
    zeta, ups = H(g["challenges"]["zeta"]), H(g["challenges"]["upsilon"])
    srs_pts = util.plonk_test_srs(oid, 7, 2)
    polys = K.circuit_polynomials(srs_pts)
    r4 = K.round_4(polys, zeta, evaluate=_evaluator(device))
    for name, want in g["round_4"].items():
        if not name.startswith("_"):
            assert r4[name] == H(want), name
    srs = msm.Srs(msm.BLS12381Curve, srs_pts)
    try:
        ps = K.round_5_polynomials(polys, r4, zeta)
        arrs = [mont(p, r) for p in ps]
        zw = zeta * K.omega() % r
        if device:
            t = [torch.from_numpy(a.view(np.int64)).cuda() for a in arrs]
            w1, evs = kzg.open_batch_device(srs, t, [len(p) for p in ps], mont([zeta], r)[0], mont([ups], r)[0])
            tz = torch.from_numpy(mont(polys["p_z"], r).view(np.int64)).cuda()
            w2, ev2 = kzg.open_device(srs, tz, len(polys["p_z"]), mont([zw], r)[0])
        else:
            w1, evs = kzg.open_batch(srs, arrs, mont([zeta], r)[0], mont([ups], r)[0])
            w2, ev2 = kzg.open(srs, mont(polys["p_z"], r), mont([zw], r)[0])
        assert O.point_to_affine_ints(oid, w1) == tuple(H(v) for v in g["round_5"]["w_zeta_1"])
        assert O.point_to_affine_ints(oid, w2) == tuple(H(v) for v in g["round_5"]["w_zeta_omega_1"])
        assert unmont(evs, r) == [K.horner(p, zeta) for p in ps]
        assert unmont(ev2.reshape(1, 4), r)[0] == H(g["round_4"]["z_zeta_omega"])
    finally:
        srs.close()


def test_device_form_on_a_side_stream_and_two_threads_on_one_handle():
    import torch
    from lambda_elliptic_curves_amd import kzg, msm
    crv, oid = util.curve_pairs()["bls12_381_g1"]
    r = D.P_FR381
    _, points = util.msm_case(oid, 8192, 17)
    srs = msm.Srs(crv, points)
    cases = [_canon_case(r, n, 500 + n) for n in (8193, 5000, 3001, 7777)]
    want = []
    for a, x in cases:
        q, _ = K.ruffini(a, x, r)
        want.append(_proof_aff(oid, O.parallel_msm_with(oid, O.ints_to_array(q, 4), points[:len(q)], 10, util.host_threads())))
    try:
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            a, x = cases[0]
            t = torch.from_numpy(mont(a, r).view(np.int64)).to("cuda", non_blocking=False)
            proof, _ = kzg.open_device(srs, t, len(a), mont([x], r)[0], stream=s.cuda_stream)
        assert _proof_aff(oid, proof) == want[0]

        def work(i):
            a, x = cases[i]
            out = []
            for _ in range(3):
                proof, _ = kzg.open(srs, mont(a, r), mont([x], r)[0])
                out.append(_proof_aff(oid, proof))
            return out
        with ThreadPoolExecutor(2) as ex:
            res = list(ex.map(work, [1, 2]))
        assert res[0] == [want[1]] * 3 and res[1] == [want[2]] * 3
    finally:
        srs.close()
