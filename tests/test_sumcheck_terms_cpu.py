"""The eq table and the sumcheck round over an eq-weighted sum of products without a GPU: the Python restatement
(tests/sumcheck_terms_ref.py) with its verifier on an honest and a tampered transcript, the exported symbols, and every
argument check of the four entry points (lw_multilinear_eq_table*, lw_sumcheck_terms_round*), which run before any device
is touched."""
import ctypes as C
import hashlib

import numpy as np
import pytest

from tests import multilinear_ref as M
from tests import sumcheck_terms_ref as T

FIELDS = sorted(M.MODULI)
SYMBOLS = ("lw_multilinear_eq_table", "lw_multilinear_eq_table_device", "lw_sumcheck_terms_round", "lw_sumcheck_terms_round_device")


def _rand(p, n, seed):
    rng = np.random.default_rng(seed)
    return [int.from_bytes(rng.bytes(40), "big") % p for _ in range(n)]


def _challenge(F):
    def ch(g):
        h = hashlib.sha3_256(b"".join(int(v).to_bytes(32, "big") for v in g)).digest()
        return int.from_bytes(h, "big") % F.p
    return ch


def test_chis_is_the_product_of_eq_factors():
    F = M.Fld(M.P_STARK252, True)
    for n in range(0, 6):
        r = _rand(F.p, n, n)
        w = M.chis(F, r)
        for i in range(1 << n):
            bits = [F.one if (i >> (n - 1 - j)) & 1 else 0 for j in range(n)]
            assert w[i] == T.eq_closed_form(F, r, bits)


@pytest.mark.parametrize("name", FIELDS)
@pytest.mark.parametrize("has_eq", [False, True])
@pytest.mark.parametrize("m", [1, 2, 3, 4])
def test_verifier_accepts_honest_and_rejects_tampered(name, m, has_eq):
    F = M.Fld(M.MODULI[name], True)
    n = 3
    tables = [_rand(F.p, 1 << n, 10 * n + k) for k in range(m)]
    eq = M.chis(F, _rand(F.p, n, 99)) if has_eq else None
    for tag, terms in T.term_lists(F, m, _rand(F.p, 3, 7)).items():
        D = T.degree(terms, has_eq)
        claimed, rounds, point, final = T.prove(F, tables, terms, _challenge(F), eq)
        assert claimed == T.cube_sum(F, tables, terms, eq), tag
        assert len(rounds) == n and all(len(g) == D + 1 for g in rounds), tag
        every = tables + ([eq] if has_eq else [])
        assert final == [M.evaluate(F, X, point) for X in every], tag
        assert T.verify(F, terms, has_eq, claimed, rounds, point, final), tag
        for i in range(n):
            for u in range(D + 1):
                bad = [list(g) for g in rounds]
                bad[i][u] = (bad[i][u] + 1) % F.p
                assert not T.verify(F, terms, has_eq, claimed, bad, point, final), (tag, i, u)
        assert not T.verify(F, terms, has_eq, (claimed + 1) % F.p, rounds, point, final), tag


@pytest.mark.parametrize("name", FIELDS)
def test_one_product_term_is_the_product_round(name):
    # without eq and with one term over all tables the composed round is multilinear_ref.round_poly
    F = M.Fld(M.MODULI[name], True)
    for k in (1, 2, 3):
        tables = [_rand(F.p, 16, 5 * k + i) for i in range(k)]
        assert T.round_poly(F, tables, [(None, tuple(range(k)))]) == M.round_poly(F, tables)


def test_symbols_are_exported_and_the_functions_are_public():
    import lambda_elliptic_curves_amd as pkg
    from lambda_elliptic_curves_amd import _lib
    L = _lib.lib()
    for sym in SYMBOLS:
        assert sym in _lib.EXPORTS and hasattr(L, sym)
        assert getattr(L, sym).argtypes is not None
    for fn in ("eq_table", "eq_table_device", "sumcheck_terms_round", "sumcheck_terms_round_device", "sumcheck_terms_prove_device"):
        assert callable(getattr(pkg.multilinear, fn))


def test_argument_checks_do_not_need_a_device():
    from lambda_elliptic_curves_amd import _lib
    L = C.CDLL(_lib.LIB_PATH)   # a handle of its own: plain ctypes arguments, no argtypes
    buf = np.zeros(8192, np.uint8)
    base = (buf.ctypes.data + 63) & ~63
    at = lambda off: C.c_void_p(base + off)
    A, B, Cc, D, E, Q, OUT, N = at(0), at(512), at(1024), at(1536), at(2048), at(2560), at(3072), C.c_void_p(None)
    ODD = at(4096 + 8)              # not 16-byte aligned
    NEAR = at(64)                   # inside a table of 2^2 elements at A
    i, u32 = C.c_int, C.c_uint32
    S, FR, BB = i(0), i(1), i(2)
    arr = lambda *ps: (C.c_void_p * len(ps))(*[p.value for p in ps])
    masks = lambda *ms: (C.c_uint32 * len(ms))(*ms)
    eqh = lambda f, pt, n, out: L.lw_multilinear_eq_table(f, pt, u32(n), out)
    eqd = lambda f, pt, n, out: L.lw_multilinear_eq_table_device(f, pt, u32(n), out, N)
    rdh = lambda f, tabs, k, eq, ms, cs, nt, n, rp, out: L.lw_sumcheck_terms_round(f, tabs, u32(k), eq, ms, cs, u32(nt), u32(n), rp, out)
    rdd = lambda f, tabs, k, eq, ms, cs, nt, n, rp, out: L.lw_sumcheck_terms_round_device(f, tabs, u32(k), eq, ms, cs, u32(nt), u32(n), rp, out, N)
    four = arr(A, B, Cc, D)
    cases = []
    for tag, e, r in (("", eqh, rdh), ("_device", eqd, rdd)):
        cases += [
            ("eq%s field" % tag, lambda e=e: e(BB, Q, 2, OUT)),
            ("eq%s point null" % tag, lambda e=e: e(S, N, 2, OUT)),
            ("eq%s out null" % tag, lambda e=e: e(FR, Q, 2, N)),
            ("eq%s out null, no variable" % tag, lambda e=e: e(S, N, 0, N)),
            ("eq%s 31 variables" % tag, lambda e=e: e(S, Q, 31, OUT)),
            ("terms%s field" % tag, lambda r=r: r(BB, arr(A), 1, N, masks(1), N, 1, 2, N, OUT)),
            ("terms%s tables null" % tag, lambda r=r: r(S, N, 1, N, masks(1), N, 1, 2, N, OUT)),
            ("terms%s table null" % tag, lambda r=r: r(S, arr(A, N), 2, N, masks(3), N, 1, 2, N, OUT)),
            ("terms%s masks null" % tag, lambda r=r: r(FR, arr(A), 1, N, N, N, 1, 2, N, OUT)),
            ("terms%s out null" % tag, lambda r=r: r(FR, arr(A), 1, N, masks(1), N, 1, 2, N, N)),
            ("terms%s no table" % tag, lambda r=r: r(S, arr(A), 0, N, masks(1), N, 1, 2, N, OUT)),
            ("terms%s five tables" % tag, lambda r=r: r(S, arr(A, B, Cc, D, E), 5, N, masks(1), N, 1, 2, N, OUT)),
            ("terms%s no term" % tag, lambda r=r: r(S, arr(A), 1, N, masks(1), N, 0, 2, N, OUT)),
            ("terms%s nine terms" % tag, lambda r=r: r(S, arr(A), 1, N, masks(*[1] * 9), N, 9, 2, N, OUT)),
            ("terms%s zero mask" % tag, lambda r=r: r(S, arr(A, B), 2, N, masks(3, 0), N, 2, 2, N, OUT)),
            ("terms%s mask bit above the tables" % tag, lambda r=r: r(S, arr(A, B), 2, N, masks(1, 4), N, 2, 2, N, OUT)),
            ("terms%s mask bit far above the tables" % tag, lambda r=r: r(S, four, 4, N, masks(1 << 31), N, 1, 2, N, OUT)),
            ("terms%s mask of four bits" % tag, lambda r=r: r(FR, four, 4, E, masks(7, 15), N, 2, 2, N, OUT)),
            ("terms%s 31 variables" % tag, lambda r=r: r(S, arr(A), 1, N, masks(1), N, 1, 31, N, OUT)),
            ("terms%s no variable" % tag, lambda r=r: r(S, arr(A), 1, N, masks(1), N, 1, 0, N, OUT)),
            ("terms%s fused, one variable" % tag, lambda r=r: r(S, arr(A), 1, E, masks(1), Q, 1, 1, Q, OUT)),
            ("terms%s same table twice" % tag, lambda r=r: r(S, arr(A, A), 2, N, masks(3), N, 1, 2, N, OUT)),
            ("terms%s tables overlap" % tag, lambda r=r: r(FR, arr(A, B, NEAR), 3, N, masks(7), N, 1, 2, Q, OUT)),
            ("terms%s eq is a table" % tag, lambda r=r: r(S, arr(A, B), 2, B, masks(3), N, 1, 2, N, OUT)),
            ("terms%s eq overlaps a table" % tag, lambda r=r: r(FR, arr(A, B), 2, NEAR, masks(3), Q, 1, 2, Q, OUT)),
        ]
    cases += [
        ("eq_device misaligned out", lambda: eqd(S, Q, 2, ODD)),
        ("terms_device misaligned table", lambda: rdd(S, arr(A, ODD), 2, N, masks(3), N, 1, 2, N, OUT)),
        ("terms_device misaligned eq", lambda: rdd(S, arr(A, B), 2, ODD, masks(3), N, 1, 2, N, OUT)),
    ]
    got = {name: call() for name, call in cases}
    assert got == {name: _lib.ERR_BAD_ARG for name, _ in cases}


def test_eq_table_of_no_variable_needs_no_device_and_nothing_else_falls_back():
    import torch
    from lambda_elliptic_curves_amd import errors, fft, multilinear
    for F, p in ((fft.Stark252PrimeField, M.P_STARK252), (fft.FrField, M.P_FR381)):
        one = np.frombuffer(((1 << 256) % p).to_bytes(32, "big"), dtype=">u8").astype(np.uint64)
        assert np.array_equal(multilinear.eq_table(F, []), one.reshape(1, 4))
    if torch.cuda.is_available():
        return
    F = fft.Stark252PrimeField
    tab, tab2 = np.ones((4, 4), np.uint64), np.ones((4, 4), np.uint64)
    with pytest.raises(errors.HipError):
        multilinear.eq_table(F, np.ones((2, 4), np.uint64))
    with pytest.raises(errors.HipError):
        multilinear.sumcheck_terms_round(F, [tab], [(None, (0,))])
    with pytest.raises(errors.HipError):
        multilinear.sumcheck_terms_round(F, [tab], [(tab[0], (0,))], eq=tab2, r_prev=tab[0])


def test_both_rounds_report_bad_tables_alike():
    """lw_sumcheck_round and lw_sumcheck_terms_round check their tables with one helper: the same bad arguments give both
    the same status and message, host and device forms.  The texts are the ones the two entry points had when each still
    carried its own copy of the checks."""
    from lambda_elliptic_curves_amd import _lib
    L = C.CDLL(_lib.LIB_PATH)
    L.lw_hip_last_error.restype = C.c_char_p
    buf = np.zeros(8192, np.uint8)
    base = (buf.ctypes.data + 63) & ~63
    at = lambda off: C.c_void_p(base + off)
    A, B, NEAR, Q, OUT, N = at(0), at(512), at(64), at(2560), at(3072), C.c_void_p(None)   # NEAR: inside 2^2 elements at A
    u32, S = C.c_uint32, C.c_int(0)
    arr = lambda *ps: (C.c_void_p * len(ps))(*[p.value for p in ps])
    one_term = (C.c_uint32 * 1)(3)   # the product of both tables
    cases = [   # tables, n_vars, r_prev, message
        (arr(A, N), 2, N, b"table 1: null or misaligned buffer"),
        (arr(A, NEAR), 2, N, b"tables 0 and 1 overlap"),
        (arr(A, B), 31, N, b"31 variables: at most 30"),
        (arr(A, B), 1, Q, b"1 variables: a round needs 1, a fused round 2"),
    ]
    for tabs, n, rp, msg in cases:
        calls = [
            lambda: L.lw_sumcheck_round(S, tabs, u32(2), u32(n), rp, OUT),
            lambda: L.lw_sumcheck_round_device(S, tabs, u32(2), u32(n), rp, OUT, N),
            lambda: L.lw_sumcheck_terms_round(S, tabs, u32(2), N, one_term, N, u32(1), u32(n), rp, OUT),
            lambda: L.lw_sumcheck_terms_round_device(S, tabs, u32(2), N, one_term, N, u32(1), u32(n), rp, OUT, N),
        ]
        for i, call in enumerate(calls):
            assert (call(), L.lw_hip_last_error()) == (_lib.ERR_BAD_ARG, msg), (msg, i)
