"""The DEEP composition polynomial without a device: stark.deep_terms (gamma order, index-based points) and the formula the
library evaluates, sum_j quot(sum_k w[k][j] p_k, x_j), against the term-by-term restatement of the reference
(tests/deep_kat.py); every argument check of lw_stark_deep_composition[_device] through a plain ctypes handle."""
import ctypes as C
import itertools

import numpy as np
import pytest

from oracle import bigint_def as D
from tests import deep_kat as K
from tests import util

MODULI = {"stark252": D.P_STARK252, "fr381": D.P_FR381}


def fld(name):
    from lambda_elliptic_curves_amd import fft
    return {"stark252": fft.Stark252PrimeField, "fr381": fft.FrField}[name]


def rand_polys(name, lens, seed):
    p = MODULI[name]
    return [K.unmont(util.rand_elems(name, n, seed + 17 * i), p) if n else [] for i, n in enumerate(lens)]


def test_package_moduli_are_the_fields():
    from lambda_elliptic_curves_amd import stark
    assert stark.MODULI[fld("stark252").field] == D.P_STARK252
    assert stark.MODULI[fld("fr381").field] == D.P_FR381


@pytest.mark.parametrize("name", ["stark252", "fr381"])
def test_deep_terms_and_formula_equal_the_literal_restatement(name):
    from lambda_elliptic_curves_amd import stark
    p, F = MODULI[name], fld(name)
    rng = np.random.default_rng(5)
    length_sets = [[40, 33, 0, 1, 64], [1, 0, 7, 2, 9], [64, 64, 64, 64, 64], [3, 50, 17, 0, 1]]
    case = 0
    for C_, T, P_ in itertools.product((1, 2, 5), (1, 3, 4), (1, 2, 4)):
        lens = length_sets[case % len(length_sets)]
        trace = rand_polys(name, [lens[(i + case) % 5] for i in range(C_)], 100 * case)
        parts = rand_polys(name, [lens[(i + 2 * case + 1) % 5] for i in range(P_)], 100 * case + 50)
        case += 1
        z, g, gamma = (int(v) for v in K.unmont(util.rand_elems(name, 3, 900 + case), p))
        want = K.deep_literal(trace, parts, z, g, T, gamma, p)
        pts_a, w_a = stark.deep_terms(F, C_, P_, T, K.mont([z], p)[0], K.mont([g], p)[0], K.mont([gamma], p)[0])
        assert pts_a.shape == (T + 1, 4) and w_a.shape == (C_ + P_, T + 1, 4) and pts_a.dtype == np.uint64
        pts = K.unmont(pts_a, p)
        w = [K.unmont(row, p) for row in w_a]
        # the index-based points and the gamma order, stated independently
        assert pts == [pow(g, r, p) * z % p for r in range(T)] + [pow(z, P_, p)]
        for j in range(C_):
            assert w[j] == [pow(gamma, j * T + r, p) for r in range(T)] + [0]
        for i in range(P_):
            assert w[C_ + i] == [0] * T + [pow(gamma, C_ * T + i, p)]
        got = K.deep_formula(trace + parts, pts, w, p)
        assert K.strip(got) == want, (C_, T, P_)
        n = max(len(a) for a in trace + parts)
        assert len(got) == max(0, n - 1)
        assert K.strip(K.deep_terms_literal(trace + parts, pts, w, p)) == want


def _handle():
    from lambda_elliptic_curves_amd import _lib
    return C.CDLL(_lib.LIB_PATH), _lib


def test_argument_checks_need_no_device():
    L, _lib = _handle()
    buf = np.zeros(8192, np.uint8)
    b0 = (buf.ctypes.data + 63) & ~63
    A, B, OUT, N = C.c_void_p(b0), C.c_void_p(b0 + 1024), C.c_void_p(b0 + 4096), C.c_void_p(None)
    pts = np.ones((2, 4), np.uint64)
    w = np.ones((2 * 2, 4), np.uint64)
    PT, W = C.c_void_p(pts.ctypes.data), C.c_void_p(w.ctypes.data)
    i, u32, sz = C.c_int, C.c_uint32, C.c_size_t
    S, FR, BB = i(0), i(1), i(2)
    ln = sz(77)
    LN = C.byref(ln)

    def tab(*ptrs):
        return (C.c_void_p * len(ptrs))(*ptrs)

    def lens(*v):
        return (sz * len(v))(*v)

    dev = lambda f, polys, ls, k, points, m, weights, out, out_len=N, evals=N: L.lw_stark_deep_composition_device(
        f, polys, ls, u32(k), points, u32(m), weights, out, out_len, evals, N)
    host = lambda f, polys, ls, k, points, m, weights, out, out_len=N, evals=N: L.lw_stark_deep_composition(
        f, polys, ls, u32(k), points, u32(m), weights, out, out_len, evals)
    two, l88 = tab(A, B), lens(8, 8)
    cases = []
    for name, fn in (("host", host), ("device", dev)):
        cases += [
            (name + " field", lambda fn=fn: fn(BB, two, l88, 2, PT, 2, W, OUT), _lib.ERR_BAD_ARG),
            (name + " m = 0", lambda fn=fn: fn(S, two, l88, 2, PT, 0, W, OUT), _lib.ERR_BAD_ARG),
            (name + " null points", lambda fn=fn: fn(S, two, l88, 2, N, 2, W, OUT), _lib.ERR_BAD_ARG),
            (name + " null weights", lambda fn=fn: fn(FR, two, l88, 2, PT, 2, N, OUT), _lib.ERR_BAD_ARG),
            (name + " null table", lambda fn=fn: fn(S, N, l88, 2, PT, 2, W, OUT), _lib.ERR_BAD_ARG),
            (name + " null lens", lambda fn=fn: fn(S, two, N, 2, PT, 2, W, OUT), _lib.ERR_BAD_ARG),
            (name + " null polynomial", lambda fn=fn: fn(S, tab(A, None), l88, 2, PT, 2, W, OUT), _lib.ERR_BAD_ARG),
            (name + " null out", lambda fn=fn: fn(S, two, l88, 2, PT, 2, W, N), _lib.ERR_BAD_ARG),
            (name + " too long", lambda fn=fn: fn(S, two, lens(8, (1 << 36) + 1), 2, PT, 2, W, OUT), _lib.ERR_ALLOC),
        ]
    cases += [
        ("device misaligned polynomial", lambda: dev(S, tab(A, C.c_void_p(b0 + 1032)), l88, 2, PT, 2, W, OUT), _lib.ERR_BAD_ARG),
        ("device misaligned out", lambda: dev(S, two, l88, 2, PT, 2, W, C.c_void_p(b0 + 4104)), _lib.ERR_BAD_ARG),
        ("device out on a polynomial", lambda: dev(S, two, l88, 2, PT, 2, W, B), _lib.ERR_BAD_ARG),
        ("device out tail in a polynomial", lambda: dev(FR, two, l88, 2, PT, 2, W, C.c_void_p(b0 + 1024 - 6 * 32)), _lib.ERR_BAD_ARG),
        ("device out head in a polynomial", lambda: dev(FR, two, l88, 2, PT, 2, W, C.c_void_p(b0 + 1024 + 7 * 32)), _lib.ERR_BAD_ARG),
    ]
    got = {name: call() for name, call, _ in cases}
    assert got == {name: code for name, _, code in cases}
    # n <= 1 and k = 0: an empty result of length 0, LW_OK, no device
    for fn in (host, dev):
        for polys, ls, k in ((two, lens(1, 0), 2), (two, lens(0, 0), 2), (N, N, 0)):
            ln.value = 77
            assert fn(S, polys, ls, k, PT, 2, W, N, LN) == _lib.OK
            assert ln.value == 0
    # the host form hands the constants back as the values (weight 0 -> 0)
    a = np.arange(4, dtype=np.uint64) + 5
    wz = np.ones((2, 2, 4), np.uint64)
    wz[0, 1] = 0
    ev = np.full((2, 2, 4), 9, np.uint64)
    assert host(S, tab(C.c_void_p(a.ctypes.data), None), lens(1, 0), 2, PT, 2, C.c_void_p(wz.ctypes.data), N, LN,
                C.c_void_p(ev.ctypes.data)) == _lib.OK
    assert np.array_equal(ev[0, 0], a) and not ev[0, 1].any() and not ev[1].any()


def test_no_cpu_fallback_for_the_deep_composition():
    import torch
    from lambda_elliptic_curves_amd import errors, poly
    name = "stark252"
    p, F = MODULI[name], fld(name)
    polys = [util.rand_elems(name, n, 3 + n) for n in (9, 5)]
    pts = util.rand_elems(name, 2, 1)
    w = util.rand_elems(name, 4, 2)
    if not torch.cuda.is_available():
        with pytest.raises(errors.HipError):
            poly.deep_composition(F, polys, pts, w)
        return
    out, n, _ = poly.deep_composition(F, polys, pts, w)
    want = K.deep_terms_literal([K.unmont(a, p) for a in polys], K.unmont(pts, p), [K.unmont(w[:2], p), K.unmont(w[2:], p)], p)
    assert K.unmont(out, p) == want and n == len(K.strip(want))
