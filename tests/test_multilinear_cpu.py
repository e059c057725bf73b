"""Multilinear tables and the sumcheck round without a GPU: the Python restatement (tests/multilinear_ref.py) on the
reference's own vectors, its verifier on an honest and a tampered transcript, and every argument check of the six entry
points (lw_multilinear_*, lw_sumcheck_round*), which run before any device is touched."""
import ctypes as C
import hashlib

import numpy as np
import pytest

from tests import multilinear_ref as M

FIELDS = sorted(M.MODULI)


def _rand(p, n, seed):
    rng = np.random.default_rng(seed)
    return [int.from_bytes(rng.bytes(40), "big") % p for _ in range(n)]


@pytest.mark.parametrize("name", FIELDS)
@pytest.mark.parametrize("montgomery", [False, True])
def test_reference_vectors(name, montgomery):
    # dense_multilinear_poly.rs tests: evaluation at (4, 3) of [1, 2, 1, 4] is 28; [0, 0, 0, 1, 1, 1, 0, 2] at (1, 1, 1) is 2
    F = M.Fld(M.MODULI[name], montgomery)
    e = F.elem
    assert M.evaluate(F, [e(1), e(2), e(1), e(4)], [e(4), e(3)]) == e(28)
    assert M.evaluate(F, [e(v) for v in (0, 0, 0, 1, 1, 1, 0, 2)], [e(1), e(1), e(1)]) == e(2)
    assert M.evaluate(F, [e(7)], []) == e(7)


@pytest.mark.parametrize("name", FIELDS)
def test_fix_variables_of_all_is_evaluate_and_of_none_is_a_copy(name):
    F = M.Fld(M.MODULI[name], True)
    for n in range(0, 7):
        T, r = _rand(F.p, 1 << n, n), _rand(F.p, n, 100 + n)
        assert M.fix_variables(F, T, r) == [M.evaluate(F, T, r)]
        assert M.fix_variables(F, T, []) == T
        for t in range(n + 1):   # the formula of the restatement: sum_b eq(r, b) T[b 2^(n-t) + j]
            w, m = M.chis(F, r[:t]), 1 << (n - t)
            assert M.fix_variables(F, T, r[:t]) == [sum(F.mul(w[b], T[b * m + j]) for b in range(1 << t)) % F.p for j in range(m)]


def _challenge(F):
    def ch(g):
        h = hashlib.sha3_256(b"".join(int(v).to_bytes(32, "big") for v in g)).digest()
        return int.from_bytes(h, "big") % F.p
    return ch


@pytest.mark.parametrize("name", FIELDS)
@pytest.mark.parametrize("K", [1, 2, 3])
def test_verifier_accepts_honest_and_rejects_tampered(name, K):
    F = M.Fld(M.MODULI[name], True)
    for n in (1, 2, 5):
        tables = [_rand(F.p, 1 << n, 10 * n + k) for k in range(K)]
        claimed, rounds, point, final = M.prove(F, tables, _challenge(F))
        assert claimed == M.cube_sum(F, tables)
        assert len(rounds) == n and all(len(g) == K + 1 for g in rounds)
        assert final == [M.evaluate(F, T, point) for T in tables]
        assert M.verify(F, claimed, rounds, point, final)
        for i in range(n):
            for u in range(K + 1):
                bad = [list(g) for g in rounds]
                bad[i][u] = (bad[i][u] + 1) % F.p
                assert not M.verify(F, claimed, bad, point, final), (n, i, u)
        assert not M.verify(F, (claimed + 1) % F.p, rounds, point, final)
        assert not M.verify(F, claimed, rounds, point, [(final[0] + 1) % F.p] + final[1:])


def test_symbols_are_exported_and_the_module_is_public():
    import lambda_elliptic_curves_amd as pkg
    from lambda_elliptic_curves_amd import _lib
    L = _lib.lib()
    for sym in ("lw_multilinear_evaluate", "lw_multilinear_evaluate_device", "lw_multilinear_fix_variables",
                "lw_multilinear_fix_variables_device", "lw_sumcheck_round", "lw_sumcheck_round_device"):
        assert sym in _lib.EXPORTS and hasattr(L, sym)
        assert getattr(L, sym).argtypes is not None
    assert "multilinear" in pkg.__all__
    for fn in ("evaluate", "evaluate_device", "fix_variables", "fix_variables_device", "sumcheck_round", "sumcheck_round_device",
               "sumcheck_prove_device"):
        assert callable(getattr(pkg.multilinear, fn))
    assert pkg.multilinear.MODULI == {_lib.FIELD_STARK252: M.P_STARK252, _lib.FIELD_BLS12_381_FR: M.P_FR381}


def test_argument_checks_do_not_need_a_device():
    from lambda_elliptic_curves_amd import _lib
    L = C.CDLL(_lib.LIB_PATH)   # a handle of its own: plain ctypes arguments, no argtypes
    buf = np.zeros(8192, np.uint8)
    base = (buf.ctypes.data + 63) & ~63
    P, Q, OUT, N = C.c_void_p(base), C.c_void_p(base + 2048), C.c_void_p(base + 4096), C.c_void_p(None)
    ODD = C.c_void_p(base + 8)                  # not 16-byte aligned
    NEAR = C.c_void_p(base + 64)                # inside a table of 2^2 elements at P
    i, u32 = C.c_int, C.c_uint32
    S, FR, BB = i(0), i(1), i(2)
    arr = lambda *ps: (C.c_void_p * len(ps))(*[p.value for p in ps])
    ev = lambda f, tabs, k, n, pt, out: L.lw_multilinear_evaluate(f, tabs, u32(k), u32(n), pt, out)
    evd = lambda f, tabs, k, n, pt, out: L.lw_multilinear_evaluate_device(f, tabs, u32(k), u32(n), pt, out, N)
    fx = lambda f, tab, n, r, t, out: L.lw_multilinear_fix_variables(f, tab, u32(n), r, u32(t), out)
    fxd = lambda f, tab, n, r, t, out: L.lw_multilinear_fix_variables_device(f, tab, u32(n), r, u32(t), out, N)
    rd = lambda f, tabs, k, n, rp, out: L.lw_sumcheck_round(f, tabs, u32(k), u32(n), rp, out)
    rdd = lambda f, tabs, k, n, rp, out: L.lw_sumcheck_round_device(f, tabs, u32(k), u32(n), rp, out, N)
    cases = []
    for tag, e, f, r in (("", ev, fx, rd), ("_device", evd, fxd, rdd)):
        cases += [
            ("evaluate%s field" % tag, lambda e=e: e(BB, arr(P), 1, 2, Q, OUT)),
            ("evaluate%s tables null" % tag, lambda e=e: e(S, N, 1, 2, Q, OUT)),
            ("evaluate%s table null" % tag, lambda e=e: e(FR, arr(P, N), 2, 2, Q, OUT)),
            ("evaluate%s point null" % tag, lambda e=e: e(S, arr(P), 1, 2, N, OUT)),
            ("evaluate%s out null" % tag, lambda e=e: e(S, arr(P), 1, 2, Q, N)),
            ("evaluate%s 31 variables" % tag, lambda e=e: e(S, arr(P), 1, 31, Q, OUT)),
            ("evaluate%s k = 0" % tag, lambda e=e: e(S, arr(P), 0, 2, Q, OUT)),
            ("fix%s field" % tag, lambda f=f: f(BB, P, 2, Q, 1, OUT)),
            ("fix%s table null" % tag, lambda f=f: f(S, N, 2, Q, 1, OUT)),
            ("fix%s r null" % tag, lambda f=f: f(FR, P, 2, N, 1, OUT)),
            ("fix%s out null" % tag, lambda f=f: f(S, P, 2, Q, 1, N)),
            ("fix%s 31 variables" % tag, lambda f=f: f(S, P, 31, Q, 1, OUT)),
            ("fix%s t > n" % tag, lambda f=f: f(S, P, 2, Q, 3, OUT)),
            ("round%s field" % tag, lambda r=r: r(BB, arr(P), 1, 2, N, OUT)),
            ("round%s tables null" % tag, lambda r=r: r(S, N, 1, 2, N, OUT)),
            ("round%s table null" % tag, lambda r=r: r(S, arr(P, N), 2, 2, N, OUT)),
            ("round%s out null" % tag, lambda r=r: r(FR, arr(P), 1, 2, N, N)),
            ("round%s 31 variables" % tag, lambda r=r: r(S, arr(P), 1, 31, N, OUT)),
            ("round%s k = 0" % tag, lambda r=r: r(S, arr(P), 0, 2, N, OUT)),
            ("round%s k = 4" % tag, lambda r=r: r(S, arr(P, Q, OUT, P), 4, 2, N, OUT)),
            ("round%s no variable" % tag, lambda r=r: r(S, arr(P), 1, 0, N, OUT)),
            ("round%s fused, one variable" % tag, lambda r=r: r(S, arr(P), 1, 1, Q, OUT)),
            ("round%s same table twice" % tag, lambda r=r: r(S, arr(P, P), 2, 2, N, OUT)),
            ("round%s tables overlap" % tag, lambda r=r: r(FR, arr(P, Q, NEAR), 3, 2, Q, OUT)),
        ]
    cases += [
        ("evaluate_device misaligned", lambda: evd(S, arr(P, ODD), 2, 2, Q, OUT)),
        ("fix_device misaligned table", lambda: fxd(S, ODD, 2, Q, 1, OUT)),
        ("fix_device misaligned out", lambda: fxd(S, P, 2, Q, 1, ODD)),
        ("fix_device out overlaps table", lambda: fxd(S, P, 2, Q, 1, NEAR)),
        ("fix_device out is the table", lambda: fxd(FR, P, 2, Q, 2, P)),
        ("round_device misaligned", lambda: rdd(S, arr(ODD), 1, 2, N, OUT)),
    ]
    got = {name: call() for name, call in cases}
    assert got == {name: _lib.ERR_BAD_ARG for name, _ in cases}


def test_constant_needs_no_device_and_nothing_else_falls_back():
    import torch
    from lambda_elliptic_curves_amd import errors, fft, multilinear
    for F in (fft.Stark252PrimeField, fft.FrField):
        t = [np.array([[1, 2, 3, 4]], np.uint64), np.array([[5, 6, 7, 8]], np.uint64)]
        assert np.array_equal(multilinear.evaluate(F, t, []), np.concatenate(t))
    if torch.cuda.is_available():
        return
    F = fft.Stark252PrimeField
    tab = np.ones((4, 4), np.uint64)
    with pytest.raises(errors.HipError):
        multilinear.evaluate(F, [tab], np.ones((2, 4), np.uint64))
    with pytest.raises(errors.HipError):
        multilinear.fix_variables(F, tab, np.ones((1, 4), np.uint64))
    with pytest.raises(errors.HipError):
        multilinear.fix_variables(F, tab, [])
    with pytest.raises(errors.HipError):
        multilinear.sumcheck_round(F, [tab])
