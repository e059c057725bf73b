"""lw_stark_deep_composition[_device] on the device against tests/deep_kat.py, the term-by-term Python restatement of
compute_deep_composition_poly (provers/stark/src/prover.rs:643-714).  Field arithmetic is exact, so every comparison is
byte equality in the stored (Montgomery) form, except the 2^22 case, which is stated as an identity at random points.

The schedule (csrc/poly.hip) shares the division's geometry: tiles of 256 x 8 coefficients, a carry scan that gives each of
its 256 threads ceil(tiles / 256) tiles, groups of 4 points per round of launches; the sizes below straddle 8, 2048, 2^19
and the point counts 4 / 5 / 9."""
import hashlib
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from oracle import bigint_def as D
from oracle import oracle as O
from tests import deep_kat as K
from tests import util

pytestmark = pytest.mark.gpu
MODULI = {"stark252": D.P_STARK252, "fr381": D.P_FR381}
BOUNDARY_SIZES = [2, 3, 8, 9, 2047, 2048, 2049, 4097, (1 << 19) - 1, 1 << 19, (1 << 19) + 1]


def fld(name):
    from lambda_elliptic_curves_amd import fft
    return {"stark252": fft.Stark252PrimeField, "fr381": fft.FrField}[name]


def cuda(a):
    import torch
    return torch.from_numpy(a.view(np.int64)).cuda() if len(a) else torch.zeros((1, 4), dtype=torch.int64, device="cuda")


def want_general(p, polys, pts, w):
    """stored arrays -> the stored coefficient list of the literal restatement (padded to n - 1) and its stripped length"""
    k, m = len(polys), len(pts)
    wi = K.unmont(w.reshape(-1, 4), p)
    lit = K.deep_terms_literal([K.unmont(a, p) for a in polys], K.unmont(pts, p), [wi[i * m:(i + 1) * m] for i in range(k)], p)
    return K.to_ints(K.mont(lit, p)), len(K.strip(lit))


def want_evals(p, polys, pts, w):
    xs = K.unmont(pts, p)
    k, m = len(polys), len(xs)
    wz = K.to_ints(w.reshape(-1, 4))
    R = 1 << 256
    return [[K.horner(K.unmont(polys[i], p), xs[j], p) * R % p if wz[i * m + j] else 0 for j in range(m)] for i in range(k)]


@pytest.mark.parametrize("name", ["stark252", "fr381"])
def test_boundary_sizes_match_the_literal_restatement(name):
    from lambda_elliptic_curves_amd import poly
    p, F = MODULI[name], fld(name)
    for n in BOUNDARY_SIZES:
        big = n > 5000
        lens = [n // 2 + 1, n, max(1, n - 1)] if big else [n // 2, n, 0, 1, max(1, n - 1)]
        m = 2 if big else 5
        polys = [util.rand_elems(name, ln, 300 + n + i) for i, ln in enumerate(lens)]
        pts = util.rand_elems(name, m, 7 + n)
        w = util.rand_elems(name, len(lens) * m, 9 + n).reshape(len(lens), m, 4)
        w[0, 0] = 0
        want, want_len = want_general(p, polys, pts, w)
        out, got_len, ev = poly.deep_composition(F, polys, pts, w)
        assert out.shape == (n - 1, 4)
        assert K.to_ints(out) == want, (name, n)
        assert got_len == want_len
        if not big:
            assert [K.to_ints(r) for r in ev] == want_evals(p, polys, pts, w), (name, n)


@pytest.mark.parametrize("name", ["stark252", "fr381"])
def test_weight_and_point_cases(name):
    from lambda_elliptic_curves_amd import poly
    p, F = MODULI[name], fld(name)
    one = (1 << 256) % p
    lens = [4100, 2049, 300, 4100]
    polys = [K.to_ints(util.rand_elems(name, n, 60 + i)) for i, n in enumerate(lens)]
    root = int(np.random.default_rng(3).integers(2, 1 << 62)) % p          # a stored point that is a root of polynomial 1
    r = root * K.rinv(p) % p
    polys[1][0] = (-K.horner([0] + polys[1][1:], r, p)) % p
    polys = [K.to_arr(a) for a in polys]
    rnd = K.to_ints(util.rand_elems(name, 3, 5))
    # 9 points (three groups): 0, 1, -1, a duplicated pair, the root, and a column that carries no weight
    pts = K.to_arr([0, one, p - one, rnd[0], rnd[0], root, rnd[1], rnd[2], rnd[1]])
    m = 9
    w = util.rand_elems(name, len(lens) * m, 21).reshape(len(lens), m, 4)
    w[:, 6] = 0                                 # an all-zero column
    w[2, :] = 0                                 # an all-zero row
    w[0, 0], w[0, 1], w[0, 2] = K.to_arr([0])[0], K.to_arr([one])[0], K.to_arr([p - one])[0]
    w[3, 3] = 0
    want, want_len = want_general(p, polys, pts, w)
    out, got_len, ev = poly.deep_composition(F, polys, pts, w)
    assert K.to_ints(out) == want and got_len == want_len
    we = want_evals(p, polys, pts, w)
    assert [K.to_ints(row) for row in ev] == we
    assert we[1][5] == 0 and K.to_ints(w[1, 5].reshape(1, 4))[0] != 0       # the root: weight non-zero, value 0
    assert not ev[2].any() and not ev[:, 6].any()
    # every weight zero: the zero polynomial of n - 1 coefficients
    out0, len0, ev0 = poly.deep_composition(F, polys, pts, np.zeros_like(w))
    assert out0.shape == (4099, 4) and not out0.any() and len0 == 0 and not ev0.any()
    # the values are lw_poly_evaluate_device's on the same pairs
    t = [cuda(a) for a in polys]
    table = poly.evaluate_device(F, t, lens, pts)
    nz = w.reshape(len(lens), m, 4).any(axis=2)
    assert np.array_equal(ev[nz], table[nz])


def _stored_scalars(name, seed):
    z, g, gamma = util.rand_elems(name, 3, seed)
    return z, g, gamma


@pytest.mark.parametrize("name", ["stark252", "fr381"])
@pytest.mark.parametrize("C_,T,P_", [(2, 3, 1), (2, 3, 2)])   # Fibonacci-like, Stone-like
def test_reference_call_shapes(name, C_, T, P_):
    import torch
    from lambda_elliptic_curves_amd import stark
    p, F = MODULI[name], fld(name)
    n = 1 << 10
    trace = [util.rand_elems(name, n, 40 + i) for i in range(C_)]
    parts = [util.rand_elems(name, n - 3 * i, 80 + i) for i in range(P_)]
    z, g, gamma = _stored_scalars(name, 11)
    zi, gi, gai = (K.unmont(v.reshape(1, 4), p)[0] for v in (z, g, gamma))
    want = K.deep_literal([K.unmont(a, p) for a in trace], [K.unmont(a, p) for a in parts], zi, gi, T, gai, p)
    t_out = torch.zeros((n - 1, 4), dtype=torch.int64, device="cuda")
    got_len, tr_ev, part_ev = stark.deep_composition_poly_device(F, [cuda(a) for a in trace], [n] * C_, [cuda(a) for a in parts],
                                                                 [n - 3 * i for i in range(P_)], z, g, T, gamma, t_out)
    assert got_len == len(want)
    got = K.unmont(t_out.cpu().numpy().view(np.uint64), p)
    assert K.strip(got) == want
    assert tr_ev.shape == (C_, T, 4) and part_ev.shape == (P_, 4)
    for j in range(C_):
        assert K.unmont(tr_ev[j], p) == [K.horner(K.unmont(trace[j], p), pow(gi, r, p) * zi % p, p) for r in range(T)]
    assert K.unmont(part_ev, p) == [K.horner(K.unmont(a, p), pow(zi, P_, p), p) for a in parts]


def test_device_form_with_and_without_host_outputs():
    import torch
    from lambda_elliptic_curves_amd import poly
    name = "stark252"
    p, F = MODULI[name], fld(name)
    lens = [30000, 12345, 30000]
    polys = [util.rand_elems(name, n, 500 + i) for i, n in enumerate(lens)]
    pts = util.rand_elems(name, 5, 1)
    w = util.rand_elems(name, 15, 2).reshape(3, 5, 4)
    w[1, 4] = 0
    t = [cuda(a) for a in polys]
    t_a = torch.zeros((29999, 4), dtype=torch.int64, device="cuda")
    t_b = torch.zeros_like(t_a)
    got_len, ev = poly.deep_composition_device(F, t, lens, pts, w, t_a)
    # no host output: nothing waited for inside; the same polynomial once the stream has run.  Called twice so that the
    # second call's tables follow the first one's while those may still be in flight.
    assert poly.deep_composition_device(F, t, lens, pts, w, t_b, evals=False) is None
    assert poly.deep_composition_device(F, t, lens, pts, w, t_b, evals=False) is None
    torch.cuda.synchronize()
    assert torch.equal(t_a, t_b)
    want, want_len = want_general(p, polys, pts, w)
    assert K.to_ints(t_a.cpu().numpy().view(np.uint64)) == want and got_len == want_len
    assert [K.to_ints(r) for r in ev] == want_evals(p, polys, pts, w)
    out_h, len_h, ev_h = poly.deep_composition(F, polys, pts, w)
    assert np.array_equal(out_h, t_a.cpu().numpy().view(np.uint64)) and len_h == got_len and np.array_equal(ev_h, ev)
    # on a side stream
    s = torch.cuda.Stream()
    t_c = torch.zeros_like(t_a)
    with torch.cuda.stream(s):
        poly.deep_composition_device(F, t, lens, pts, w, t_c, stream=s.cuda_stream, evals=False)
    s.synchronize()
    assert torch.equal(t_a, t_c)


def test_scale_2_20_reference_shape():
    """C = 4, T = 3, P = 2 at 2^20 against the literal restatement (14 Python divisions of 2^20)"""
    import torch
    from lambda_elliptic_curves_amd import stark
    name = "stark252"
    p, F = MODULI[name], fld(name)
    n, C_, T, P_ = 1 << 20, 4, 3, 2
    arrs = [util.rand_elems(name, n, 700 + i) for i in range(C_ + P_)]
    z, g, gamma = _stored_scalars(name, 13)
    zi, gi, gai = (K.unmont(v.reshape(1, 4), p)[0] for v in (z, g, gamma))
    t = [cuda(a) for a in arrs]
    t_out = torch.zeros((n - 1, 4), dtype=torch.int64, device="cuda")
    got_len, _, _ = stark.deep_composition_poly_device(F, t[:C_], [n] * C_, t[C_:], [n] * P_, z, g, T, gamma, t_out)
    got = t_out.cpu().numpy().view(np.uint64)
    with ThreadPoolExecutor(util.host_threads()) as ex:
        ints = list(ex.map(lambda a: K.unmont(a, p), arrs))
    want = K.deep_literal(ints[:C_], ints[C_:], zi, gi, T, gai, p)
    assert got_len == len(want)
    assert K.to_ints(got) == K.to_ints(K.mont(want + [0] * (n - 1 - len(want)), p))


def test_2_22_identity_at_two_random_points():
    """deep(r) = sum_{k,j} w[k][j] (p_k(r) - p_k(x_j)) / (r - x_j) at two random r, every value from
    lw_poly_evaluate_device: a property check, not byte equality (a literal restatement at 2^22 costs minutes)"""
    import torch
    from lambda_elliptic_curves_amd import poly, stark
    name = "stark252"
    p, F = MODULI[name], fld(name)
    n, C_, T, P_ = 1 << 22, 4, 3, 2
    g = torch.Generator(device="cuda")
    g.manual_seed(22)
    t = []
    for _ in range(C_ + P_):
        a = torch.randint(-(1 << 63), (1 << 63) - 1, (n, 4), dtype=torch.int64, device="cuda", generator=g)
        a[:, 0] &= (1 << 58) - 1            # canonical: below 2^250 < p
        t.append(a)
    z, gg, gamma = _stored_scalars(name, 17)
    pts, w = stark.deep_terms(F, C_, P_, T, z, gg, gamma)
    t_out = torch.zeros((n - 1, 4), dtype=torch.int64, device="cuda")
    got_len, ev = poly.deep_composition_device(F, t, [n] * (C_ + P_), pts, w, t_out)
    assert 0 < got_len <= n - 1
    rs = util.rand_elems(name, 2, 99)
    at_x = poly.evaluate_device(F, t, [n] * (C_ + P_), pts)
    nz = w.any(axis=2)
    assert np.array_equal(ev[nz], at_x[nz]) and not ev[~nz].any()
    at_r = poly.evaluate_device(F, t, [n] * (C_ + P_), rs)
    deep_r = poly.evaluate_device(F, [t_out], [n - 1], rs)[0]
    xs = K.unmont(pts, p)
    wi = [K.unmont(row, p) for row in w]
    for i, r in enumerate(K.unmont(rs, p)):
        pr = K.unmont(at_r[:, i], p)
        total = 0
        for k in range(C_ + P_):
            pk_x = K.unmont(at_x[k], p)
            for j in range(T + 1):
                if wi[k][j]:
                    total = (total + wi[k][j] * (pr[k] - pk_x[j]) * pow(r - xs[j], -1, p)) % p
        assert K.unmont(deep_r[i].reshape(1, 4), p)[0] == total


def _transcript_challenge(state):
    return int.from_bytes(hashlib.sha256(state).digest()[:31], "big")


@pytest.mark.parametrize("log_coeffs,blowup_log", [(12, 3), (16, 1)])
def test_deep_polynomial_feeds_the_fri_commit_phase(log_coeffs, blowup_log):
    """round 4 (prover.rs:575-594): the device's DEEP polynomial goes unchanged into commit_phase; every layer root and the
    last value equal the chain the checker builds from the Python DEEP polynomial."""
    import torch
    from lambda_elliptic_curves_amd import merkle, stark
    name = "stark252"
    f, p, F = O.F_STARK252, MODULI[name], fld(name)
    n, C_, T, P_ = 1 << log_coeffs, 2, 3, 2
    arrs = [util.rand_elems(name, n, 1200 + log_coeffs + i) for i in range(C_ + P_)]
    z, g, gamma = _stored_scalars(name, 19)
    zi, gi, gai = (K.unmont(v.reshape(1, 4), p)[0] for v in (z, g, gamma))
    t = [cuda(a) for a in arrs]
    t_out = torch.zeros((n - 1, 4), dtype=torch.int64, device="cuda")
    got_len, _, _ = stark.deep_composition_poly_device(F, t[:C_], [n] * C_, t[C_:], [n] * P_, z, g, T, gamma, t_out)
    ints = [K.unmont(a, p) for a in arrs]
    want = K.deep_literal(ints[:C_], ints[C_:], zi, gi, T, gai, p)
    assert got_len == len(want) == n - 1
    domain = n << blowup_log
    number_layers = log_coeffs + 1
    h = 3
    state = {"s": b"deep-fri-test", "zetas": []}

    def sample_zeta():
        zt = _transcript_challenge(state["s"])
        state["zetas"].append(zt)
        state["s"] = hashlib.sha256(state["s"] + b"z").digest()
        return O.elems_to_mont(f, [zt])[0]

    def append_root(root):
        state["s"] = hashlib.sha256(state["s"] + root).digest()

    def offset_sq(k):
        return O.elems_to_mont(f, [pow(h, 1 << k, p)])[0]

    t_last, layers = merkle.fri_commit_phase_device(F, number_layers, t_out, got_len, sample_zeta, append_root, offset_sq, domain)
    assert len(layers) == number_layers - 1
    poly_ = K.mont(want, p)
    dom = domain
    for k, (t_ev, t_nodes, root, dsize) in enumerate(layers, start=1):
        zeta = O.elems_to_mont(f, [state["zetas"][k - 1]])[0]
        poly_ = O.fri_fold_twice(f, poly_, zeta)
        dom //= 2
        assert dsize == dom
        ev = O.bit_reverse_permute(f, O.evaluate_fft(f, poly_, 1, dom, offset_sq(k)))
        leaves = ev.reshape(dom // 2, 2, 4)
        exp_nodes = O.merkle_commit_columns(np.ascontiguousarray(leaves.transpose(1, 0, 2)), bit_reverse=False,
                                            threads=util.host_threads())
        assert root == exp_nodes[0].tobytes(), f"layer {k} root"
    last = O.fri_fold_twice(f, poly_, O.elems_to_mont(f, [state["zetas"][-1]])[0], strip=False)
    assert last.shape[0] == 1
    assert np.array_equal(t_last.cpu().numpy().view(np.uint64)[0], last[0])
