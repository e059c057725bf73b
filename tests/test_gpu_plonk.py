"""PLONK rounds 1-3 on the device (lw_plonk_*, lambda_elliptic_curves_amd/plonk.py) against the reference's hard-coded
commitments and against the Python restatement (tests/plonk_rounds_ref.py), bit for bit.

Round 2's scan (lambda_elliptic_curves_amd/csrc/plonk.hip): PLONK_THREADS = 256 threads x PLONK_E = 2 rows make a tile of
512 rows; the carry kernel has PLONK_TOP = 64 threads, each owning ceil(tiles / 64) consecutive tiles.  So the sizes at
which a further level comes into play are
    n = 512     one full tile (every thread of the tile scan holds two live rows),
    n = 1024    two tiles: the first carry between tiles,
    n = 2^16    128 tiles: the first size at which a carry thread owns more than one tile,
and they are what ROUND2_SIZES adds to the small and the required ones."""
import numpy as np
import pytest

from oracle import oracle as O
from tests import plonk_kat_round45 as K45
from tests import plonk_rounds_ref as R
from tests import util

pytestmark = pytest.mark.gpu
H = lambda s: int(s, 16)
TILE = 512
ROUND2_SIZES = [1, 2, 4, TILE, 1 << 10, 1 << 16]
ROUND3_CASES = [(1, 1), (2, 0), (4, 4), (8, 1), (64, 0), (64, 64), (1 << 12, 1)]   # (n, n_pub); n = 4: 4n < 3 (n + 2)


def fld(f):
    from lambda_elliptic_curves_amd import fft
    return {"stark252": fft.Stark252PrimeField, "fr381": fft.FrField}[f.name]


def circuit_of(c):
    from lambda_elliptic_curves_amd import plonk
    f = c["field"]
    m = lambda cols: [R.mont(f, col) for col in cols]
    return plonk.Circuit(fld(f), c["n"], R.mont(f, [c["k1"]])[0], m(c["q_coeffs"]), m(c["s_coeffs"]), m(c["s_lagrange"]))


def witness_arr(c):
    return np.concatenate([R.mont(c["field"], w) for w in c["witness"]])


def cuda(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).cuda()


def host(t):
    return t.cpu().numpy().view(np.uint64)


def one(f, v):
    return R.mont(f, [v])[0]


def blocks(f, arr):
    return [R.unmont(f, b) for b in np.asarray(arr)]


# ---------------------------------------------------------------- the reference's own test circuit
def test_device_rounds_1_to_5_reproduce_the_reference_held_commitments_and_openings():
    import json
    import os
    from lambda_elliptic_curves_amd import kzg, msm
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_kats.json")) as fh:
        kats = json.load(fh)
    c = R.reference_test_circuit()
    f, n, oid = c["field"], c["n"], O.C_BLS12_381_G1
    srs_pts = util.plonk_test_srs(oid, 7, 2)
    srs = msm.Srs(msm.BLS12381Curve, srs_pts)
    try:
        with circuit_of(c) as cir:
            t_w = cuda(witness_arr(c))
            t_abc = cir.round1_device(t_w)
            t_z = cir.round2_device(t_w, one(f, c["beta"]), one(f, c["gamma"]))
            t_t = cir.round3_device(t_abc, t_z, R.mont(f, c["public_input"]), one(f, c["beta"]), one(f, c["gamma"]), one(f, c["alpha"]))
            commit = lambda t: O.point_to_affine_ints(oid, srs.msm_fr_device(t, t.shape[0]))
            got = {"a_1": commit(t_abc[0]), "b_1": commit(t_abc[1]), "c_1": commit(t_abc[2]), "z_1": commit(t_z),
                   "t_lo_1": commit(t_t[0]), "t_mid_1": commit(t_t[1]), "t_hi_1": commit(t_t[2])}
            want = {k + "_1": v for k, v in kats["plonk_round_1_commitments"]["expected"].items()}
            want.update(kats["plonk_round_2_3_commitments"]["expected"])
            assert set(got) == set(want)
            for name, v in want.items():
                assert got[name] == (tuple(H(x) for x in v) if v else None), name
            # rounds 4-5 on the resident blocks: p_a, p_b, p_c, p_z stay where rounds 1-2 left them
            g = K45.golden()
            zeta, ups = H(g["challenges"]["zeta"]), H(g["challenges"]["upsilon"])
            names = ["ql", "qr", "qo", "qm", "qc", "s1", "s2", "s3"]
            polys = {k: R.strip(f, v) for k, v in zip(names, c["q_coeffs"] + c["s_coeffs"])}
            polys.update({k: R.strip(f, v) for k, v in zip(["p_a", "p_b", "p_c"], blocks(f, host(t_abc)))})
            polys["p_z"] = R.strip(f, R.unmont(f, host(t_z)))
            polys.update({k: R.strip(f, v) for k, v in zip(["t_lo", "t_mid", "t_hi"], blocks(f, host(t_t)))})
            r4 = K45.round_4(polys, zeta)
            for name, v in g["round_4"].items():
                if not name.startswith("_"):
                    assert r4[name] == H(v), name
            ps = K45.round_5_polynomials(polys, r4, zeta)
            t_ps = [cuda(R.mont(f, ps[0])), cuda(R.mont(f, ps[1])), t_abc[0], t_abc[1], t_abc[2], cuda(R.mont(f, ps[5])), cuda(R.mont(f, ps[6]))]
            lens = [len(ps[0]), len(ps[1]), n + 2, n + 2, n + 2, len(ps[5]), len(ps[6])]
            w1, evs = kzg.open_batch_device(srs, t_ps, lens, one(f, zeta), one(f, ups))
            w2, ev2 = kzg.open_device(srs, t_z, n + 3, one(f, zeta * K45.omega() % f.p))
            assert O.point_to_affine_ints(oid, w1) == tuple(H(v) for v in g["round_5"]["w_zeta_1"])
            assert O.point_to_affine_ints(oid, w2) == tuple(H(v) for v in g["round_5"]["w_zeta_omega_1"])
            assert R.unmont(f, evs) == [K45.horner(p, zeta) for p in ps]
            assert R.unmont(f, ev2.reshape(1, 4))[0] == H(g["round_4"]["z_zeta_omega"])
    finally:
        srs.close()


# ---------------------------------------------------------------- round 1
@pytest.mark.parametrize("name", ["fr381", "stark252"])
def test_round_1_matches_the_restatement(name):
    f = R.FIELDS[name]
    for n, bl in ((1, [5, 6, 7, 8, 9, 10]), (2, None), (8, [f.p - 1, 2, 3, f.p - 4, 5, 6]), (1 << 10, [1, 2, 3, 4, 5, 6])):
        c = R.random_circuit(f, n, 40 + n)
        want = R.round_1(f, n, c["witness"], bl)
        with circuit_of(c) as cir:
            b = R.mont(f, bl) if bl else None
            assert blocks(f, cir.round1(witness_arr(c), b)) == want, n
            assert blocks(f, host(cir.round1_device(cuda(witness_arr(c)), b))) == want, n


# ---------------------------------------------------------------- round 2
_round2_cache = {}


def round2_case(name, n):
    """(circuit dict, blinders, reference z, reference p_z), computed once per (field, n)"""
    key = (name, n)
    if key not in _round2_cache:
        f = R.FIELDS[name]
        c = R.random_circuit(f, n, 100 + n)
        bl = [3, f.p - 2, 12345] if n in (1, 4, TILE, 1 << 16) else None
        z, p_z = R.round_2(f, n, c["k1"], c["witness"], c["s_lagrange"], c["beta"], c["gamma"], bl)
        _round2_cache[key] = (c, bl, z, p_z)
    return _round2_cache[key]


@pytest.mark.parametrize("n", ROUND2_SIZES)
@pytest.mark.parametrize("name", ["fr381", "stark252"])
def test_round_2_matches_the_restatement(name, n):
    f = R.FIELDS[name]
    c, bl, z, p_z = round2_case(name, n)
    b = R.mont(f, bl) if bl else None
    with circuit_of(c) as cir:
        tz, tp = cir.round2_device(cuda(witness_arr(c)), one(f, c["beta"]), one(f, c["gamma"]), b, z_values=True)
        assert np.array_equal(host(tz), R.mont(f, z))
        assert np.array_equal(host(tp), R.mont(f, p_z))
        if n <= 1 << 10:   # the host form agrees, and the form without z values
            hz, hp = cir.round2(witness_arr(c), one(f, c["beta"]), one(f, c["gamma"]), b)
            assert np.array_equal(hz, host(tz)) and np.array_equal(hp, host(tp))
            assert np.array_equal(host(cir.round2_device(cuda(witness_arr(c)), one(f, c["beta"]), one(f, c["gamma"]), b)), hp)


@pytest.mark.parametrize("name", ["fr381", "stark252"])
def test_round_2_zero_factors(name):
    from lambda_elliptic_curves_amd import errors
    f, n, p = R.FIELDS[name], 1 << 10, R.FIELDS[name].p
    base = R.random_circuit(f, n, 7)
    w = R.omega(f, n)
    be, ga = one(f, base["beta"]), one(f, base["gamma"])

    def with_row(i, zero_num):
        """a copy of the circuit whose row i has a zero numerator (first factor) or a zero denominator"""
        c = dict(base, witness=[list(col) for col in base["witness"]])
        eta = pow(w, i, p) if zero_num else base["s_lagrange"][0][i]
        c["witness"][0][i] = (-(base["beta"] * eta + base["gamma"])) % p
        return c

    with circuit_of(base) as cir:   # the witness changes, the circuit does not
        # a zero numerator in mid-vector is legal: z is zero from there on
        c = with_row(700, True)
        z, p_z = R.round_2(f, n, c["k1"], c["witness"], c["s_lagrange"], c["beta"], c["gamma"])
        assert z[700] != 0 and z[701] == 0 and z[-1] == 0
        hz, hp = cir.round2(witness_arr(c), be, ga)
        assert np.array_equal(hz, R.mont(f, z)) and np.array_equal(hp, R.mont(f, p_z))
        # a zero denominator in row n-1 is never read
        c = with_row(n - 1, False)
        z, p_z = R.round_2(f, n, c["k1"], c["witness"], c["s_lagrange"], c["beta"], c["gamma"])
        hz, hp = cir.round2(witness_arr(c), be, ga)
        assert np.array_equal(hz, R.mont(f, z)) and np.array_equal(hp, R.mont(f, p_z))
        # in rows 0, n-2 and on both sides of the tile boundary the reference's division fails
        for i in (0, TILE - 1, TILE, n - 2):
            c = with_row(i, False)
            with pytest.raises(ValueError):
                R.round_2(f, n, c["k1"], c["witness"], c["s_lagrange"], c["beta"], c["gamma"])
            with pytest.raises(errors.FieldError):
                cir.round2(witness_arr(c), be, ga)
            with pytest.raises(errors.FieldError):
                cir.round2_device(cuda(witness_arr(c)), be, ga)
        # the library stays usable
        _, _, z, p_z = round2_case(name, n)
        c = round2_case(name, n)[0]
    with circuit_of(c) as cir:
        hz, hp = cir.round2(witness_arr(c), one(f, c["beta"]), one(f, c["gamma"]))
        assert np.array_equal(hz, R.mont(f, z)) and np.array_equal(hp, R.mont(f, p_z))


# ---------------------------------------------------------------- round 3
def round3_inputs(f, n, n_pub, seed):
    c = R.random_circuit(f, n, seed, n_pub)
    rng = np.random.default_rng(seed + 1)
    rnd = lambda count: [int.from_bytes(rng.bytes(40), "big") % f.p for _ in range(count)]
    # blinded inputs with full-length high parts: n + 2 and n + 3 random coefficients
    return c, [rnd(n + 2) for _ in range(3)], rnd(n + 3), rnd(2)


@pytest.mark.parametrize("n,n_pub", ROUND3_CASES)
@pytest.mark.parametrize("name", ["fr381", "stark252"])
def test_round_3_matches_the_restatement(name, n, n_pub):
    f = R.FIELDS[name]
    c, p_abc, p_z, bl = round3_inputs(f, n, n_pub, 300 + n + n_pub)
    want = R.round_3(f, n, c["k1"], c["q_coeffs"], c["s_coeffs"], p_abc, p_z, c["public_input"], c["beta"], c["gamma"], c["alpha"], bl)
    if n >= 8:   # the coefficients the slices drop are there: a random "circuit" has no degree bound
        assert 4 * n > 3 * (n + 2)
    a_abc, a_z, pi = np.concatenate([R.mont(f, q) for q in p_abc]), R.mont(f, p_z), R.mont(f, c["public_input"])
    ch = [one(f, c[k]) for k in ("beta", "gamma", "alpha")]
    with circuit_of(c) as cir:
        t_abc, t_z = cuda(a_abc), cuda(a_z)
        got = cir.round3_device(t_abc, t_z, pi, *ch, blinders=R.mont(f, bl))
        assert blocks(f, host(got)) == want
        assert np.array_equal(host(t_abc), a_abc) and np.array_equal(host(t_z), a_z)   # the inputs are left alone
        if n <= 64:
            assert blocks(f, cir.round3(a_abc, a_z, pi, *ch, blinders=R.mont(f, bl))) == want
            # no blinders: the same blocks without b_0, b_1
            plain = R.round_3(f, n, c["k1"], c["q_coeffs"], c["s_coeffs"], p_abc, p_z, c["public_input"], c["beta"], c["gamma"], c["alpha"])
            assert blocks(f, cir.round3(a_abc, a_z, pi, *ch)) == plain


# ---------------------------------------------------------------- the handle
def test_two_handles_streams_and_argument_checks_on_a_live_handle():
    import ctypes as C
    import torch
    from lambda_elliptic_curves_amd import _lib as L
    from lambda_elliptic_curves_amd import errors
    fa, fb = R.FR381, R.STARK252
    ca, pa_abc, pa_z, bla = round3_inputs(fa, 64, 64, 364 + 64)
    cb, pb_abc, pb_z, blb = round3_inputs(fb, 8, 1, 300 + 8 + 1)
    wa = R.round_3(fa, 64, ca["k1"], ca["q_coeffs"], ca["s_coeffs"], pa_abc, pa_z, ca["public_input"], ca["beta"], ca["gamma"], ca["alpha"], bla)
    wb = R.round_3(fb, 8, cb["k1"], cb["q_coeffs"], cb["s_coeffs"], pb_abc, pb_z, cb["public_input"], cb["beta"], cb["gamma"], cb["alpha"], blb)
    with circuit_of(ca) as cir_a, circuit_of(cb) as cir_b:   # two handles of different n and field, live at once
        ta, tza = cuda(np.concatenate([R.mont(fa, q) for q in pa_abc])), cuda(R.mont(fa, pa_z))
        tb, tzb = cuda(np.concatenate([R.mont(fb, q) for q in pb_abc])), cuda(R.mont(fb, pb_z))
        cha = [one(fa, ca[k]) for k in ("beta", "gamma", "alpha")]
        chb = [one(fb, cb[k]) for k in ("beta", "gamma", "alpha")]
        torch.cuda.synchronize()
        s = torch.cuda.Stream()
        for _ in range(2):   # reuse across calls, alternating handles and streams
            with torch.cuda.stream(s):
                ga = cir_a.round3_device(ta, tza, R.mont(fa, ca["public_input"]), *cha, blinders=R.mont(fa, bla), stream=s.cuda_stream)
            gb = cir_b.round3_device(tb, tzb, R.mont(fb, cb["public_input"]), *chb, blinders=R.mont(fb, blb))
            s.synchronize()
            assert blocks(fa, host(ga)) == wa
            assert blocks(fb, host(gb)) == wb
        # argument checks that need a live handle: each returns its code, and the handle keeps working
        lib = L.lib()
        vp = lambda a: a.ctypes.data_as(C.c_void_p)
        pi = R.mont(fb, [1] * 9)
        out = torch.empty((3, 11, 4), dtype=torch.int64, device="cuda")
        dp = lambda t, off=0: C.c_void_p(t.data_ptr() + off)
        r3 = lambda abc, z, n_pub, o: lib.lw_plonk_round3_device(cir_b._h, abc, z, vp(pi), n_pub, vp(chb[0]), vp(chb[1]), vp(chb[2]), None, o, None)
        assert r3(dp(tb), dp(tzb), 9, dp(out)) == L.ERR_LENGTH_MISMATCH          # n_pub > n
        assert r3(dp(tb, 8), dp(tzb), 1, dp(out)) == L.ERR_BAD_ARG               # misaligned device pointers
        assert r3(dp(tb), dp(tzb, 8), 1, dp(out)) == L.ERR_BAD_ARG
        assert r3(dp(tb), dp(tzb), 1, dp(out, 8)) == L.ERR_BAD_ARG
        assert r3(None, dp(tzb), 1, dp(out)) == L.ERR_BAD_ARG                    # null pointers
        assert r3(dp(tb), dp(tzb), 1, None) == L.ERR_BAD_ARG
        assert lib.lw_plonk_round3_device(cir_b._h, dp(tb), dp(tzb), None, 1, vp(chb[0]), vp(chb[1]), vp(chb[2]), None, dp(out), None) == L.ERR_BAD_ARG
        assert lib.lw_plonk_round1_device(cir_b._h, dp(tb, 8), None, dp(out), None) == L.ERR_BAD_ARG
        assert lib.lw_plonk_round2_device(cir_b._h, dp(tb), vp(chb[0]), None, None, None, dp(out), None) == L.ERR_BAD_ARG
        assert lib.lw_plonk_round2_device(cir_b._h, dp(tb), vp(chb[0]), vp(chb[1]), None, dp(out, 8), dp(out), None) == L.ERR_BAD_ARG
        with pytest.raises(errors.LengthMismatch):
            cir_b.round3(host(tb), host(tzb), pi, *chb)
        gb = cir_b.round3_device(tb, tzb, R.mont(fb, cb["public_input"]), *chb, blinders=R.mont(fb, blb))
        assert blocks(fb, host(gb)) == wb
    # a coset on which the vanishing polynomial has a root: k1^n = 1
    for f, n in ((fa, 8), (fb, 4)):
        for k1 in (1, R.omega(f, n), R.omega(f, 4 * n)):
            with pytest.raises(errors.FieldError):
                circuit_of(dict(R.random_circuit(f, n, 1), k1=k1))
