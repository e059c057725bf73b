"""Circle FFT over Mersenne31 without a device: the restatement the GPU tests compare against (tests/circle_ref.py)
checked against the definition, and the boundary (exports, status codes, wrapper errors) of the new entry points."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from tests import circle_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = R.P
GOLDEN = json.load(open(os.path.join(ROOT, "tests", "golden", "circle_m31.json")))
SYMBOLS = ["lw_circle_evaluate_cfft", "lw_circle_interpolate_cfft", "lw_circle_evaluate_cfft_device",
           "lw_circle_interpolate_cfft_device", "lw_circle_lde_device", "lw_circle_get_twiddles"]


def _inputs(L):
    n = 1 << L
    rng = np.random.default_rng(100 + L)
    cases = [[int(v) for v in rng.integers(0, 1 << 32, n, dtype=np.uint64)],
             [0] * n, [1] * n, [P - 1] * n, [P] * n, [1 << 31] * n, [(1 << 32) - 1] * n]
    for at in (0, n - 1, n // 2):
        v = [0] * n
        v[at] = P - 1
        cases.append(v)
    return cases


# ---- the restatement
@pytest.mark.parametrize("L", range(1, 9))
def test_layered_form_is_the_naive_evaluation(L):
    for c in _inputs(L) if L <= 6 else _inputs(L)[:2]:   # the naive form is quadratic
        ev = R.evaluate_cfft(c)
        assert ev == R.evaluate_naive(c)
        assert all(0 <= v < P for v in ev)


@pytest.mark.parametrize("L", range(1, 9))
def test_interpolate_inverts_evaluate(L):
    for c in _inputs(L):
        assert R.interpolate_cfft(R.evaluate_cfft(c)) == [R.reduce_word(w) for w in c]


def test_generator_and_group():
    g = tuple(GOLDEN["generator"])
    assert g == R.GENERATOR and (g[0] * g[0] + g[1] * g[1]) % P == 1
    assert R.pmul(1 << 31, g) == (1, 0) and R.pmul(1 << 30, g) != (1, 0)   # order exactly 2^31
    for k in range(0, 6):
        assert R.pmul(1 << k, R.subgroup_generator(k)) == (1, 0)
    pts = R.coset_points(10)   # past the reference's u8
    assert len(set(pts)) == 1024 and R.padd(pts[-1], R.subgroup_generator(10)) == pts[0]


def test_golden_vectors():
    for case in GOLDEN["order_result"]:
        assert R.order_result(case["input"]) == case["expected"]
    for case in GOLDEN["order_input"]:
        assert R.order_input(case["input"]) == case["expected"]
    for case in GOLDEN["evaluations"]:
        assert R.evaluate_cfft(case["coeffs"]) == case["evals"]
        assert R.interpolate_cfft(case["evals"]) == case["coeffs"]
    for case in GOLDEN["roundtrips"]:
        assert [v % P for v in case["coeffs_as_written"]] == case["coeffs"]
        assert R.interpolate_cfft(R.evaluate_cfft(case["coeffs"])) == case["coeffs"]
    assert R.evaluate_cfft([1, 2, 3, 4]) == [32767, 2147319810, 2147450878, 163843]
    assert R.evaluate_cfft([1, 2]) == [2147483646, 3]
    assert R.interpolate_cfft([]) == []


@pytest.mark.parametrize("L", range(1, 9))
def test_twiddles_closed_form_and_lengths(L):
    ev, it = R.get_twiddles(L), R.get_twiddles(L, True)
    assert [len(layer) for layer in ev] == [1 << i for i in range(L)]             # each twice the one before
    assert [len(layer) for layer in it] == [1 << i for i in range(L - 1, -1, -1)]   # each half the one before
    for i in range(L):
        assert ev[i] == [R.twiddle_closed_form(L, i, j) for j in range(1 << i)]
        assert all(t != 0 for t in ev[i])
        assert [a * b % P for a, b in zip(ev[i], it[L - 1 - i])] == [1] * (1 << i)
    if L >= 2:   # the x-layers do not depend on the size
        assert ev[:L - 1] == R.get_twiddles(L + 1)[:L - 1]
    flat = R.flat_twiddles(L, 1)
    assert len(flat) == (1 << L) - 1 and list(flat[:1 << (L - 1)]) == it[0]


def test_numpy_form_is_the_integer_form():
    rng = np.random.default_rng(5)
    for L in (1, 2, 3, 10):
        w = rng.integers(0, 1 << 32, (2, 1 << L), dtype=np.uint64).astype(np.uint32)
        w[0, 0], w[1, -1] = P, 0xFFFFFFFF
        assert R.np_evaluate_cfft(w).tolist() == [R.evaluate_cfft(row) for row in w]
        assert R.np_interpolate_cfft(w).tolist() == [R.interpolate_cfft(row) for row in w]
        assert R.np_evaluate_cfft(w[0]).tolist() == R.evaluate_cfft(w[0])
    c = rng.integers(0, 1 << 32, (2, 8), dtype=np.uint64).astype(np.uint32)
    ev = R.np_evaluate_cfft(c)
    assert R.np_lde(ev, 5).tolist() == [R.evaluate_cfft([R.reduce_word(v) for v in row] + [0] * 24) for row in c]


# ---- the boundary
def test_symbols_are_exported_and_declared():
    from lambda_elliptic_curves_amd import _lib
    L = _lib.lib()
    header = open(os.path.join(ROOT, "include", "lw_hip.h")).read()
    ffi = open(os.path.join(ROOT, "rust-shim", "src", "ffi.rs")).read()
    for sym in SYMBOLS:
        assert sym in _lib.EXPORTS and hasattr(L, sym)
        assert sym + "(" in header and "pub fn " + sym + "(" in ffi


def test_status_codes_need_no_device():
    from lambda_elliptic_curves_amd import _lib
    L = C.CDLL(_lib.LIB_PATH)   # a handle of its own: plain ctypes arguments, no argtypes
    buf = np.zeros(1 << 12, np.uint32)
    at = lambda words: C.c_void_p(buf.ctypes.data + 4 * words)
    A, B, N = at(0), at(2048), C.c_void_p(None)
    u32, sz, i = C.c_uint32, C.c_size_t, C.c_int
    BAD, ORDER = _lib.ERR_BAD_ARG, _lib.ERR_ORDER_TOO_LARGE
    cases = []
    for name, f in (("evaluate", lambda *a: L.lw_circle_evaluate_cfft(*a)), ("interpolate", lambda *a: L.lw_circle_interpolate_cfft(*a)),
                    ("evaluate_device", lambda *a: L.lw_circle_evaluate_cfft_device(*a, N)),
                    ("interpolate_device", lambda *a: L.lw_circle_interpolate_cfft_device(*a, N))):
        cases += [
            (name + " null in", lambda f=f: f(N, B, u32(4), u32(1), sz(0)), BAD),
            (name + " null out", lambda f=f: f(A, N, u32(4), u32(1), sz(0)), BAD),
            (name + " log2n 0", lambda f=f: f(A, B, u32(0), u32(1), sz(0)), BAD),
            (name + " batch 0", lambda f=f: f(A, B, u32(4), u32(0), sz(0)), BAD),
            (name + " stride", lambda f=f: f(A, B, u32(4), u32(2), sz(15)), BAD),
            (name + " overlap", lambda f=f: f(A, at(8), u32(4), u32(1), sz(0)), BAD),
            (name + " strided overlap", lambda f=f: f(A, at(40), u32(4), u32(3), sz(20)), BAD),
            (name + " log2n 31", lambda f=f: f(A, B, u32(31), u32(1), sz(0)), ORDER),
        ]
    lde = lambda d_in, lin, sin, d_out, lout, sout, batch: L.lw_circle_lde_device(d_in, u32(lin), sz(sin), d_out, u32(lout), sz(sout), u32(batch), N)
    cases += [
        ("lde null in", lambda: lde(N, 2, 0, B, 4, 0, 1), BAD),
        ("lde null out", lambda: lde(A, 2, 0, N, 4, 0, 1), BAD),
        ("lde log2_in 0", lambda: lde(A, 0, 0, B, 4, 0, 1), BAD),
        ("lde batch 0", lambda: lde(A, 2, 0, B, 4, 0, 0), BAD),
        ("lde shrinking", lambda: lde(A, 4, 0, B, 2, 0, 1), BAD),
        ("lde in stride", lambda: lde(A, 2, 3, B, 4, 0, 2), BAD),
        ("lde out stride", lambda: lde(A, 2, 0, B, 4, 15, 2), BAD),
        ("lde overlap", lambda: lde(A, 2, 0, at(2), 4, 0, 1), BAD),
        ("lde log2_out 31", lambda: lde(A, 2, 0, B, 31, 0, 1), ORDER),
        ("twiddles log2n 0", lambda: L.lw_circle_get_twiddles(u32(0), i(0), A), BAD),
        ("twiddles null", lambda: L.lw_circle_get_twiddles(u32(3), i(0), N), BAD),
        ("twiddles config", lambda: L.lw_circle_get_twiddles(u32(3), i(2), A), BAD),
        ("twiddles log2n 31", lambda: L.lw_circle_get_twiddles(u32(31), i(0), A), ORDER),
    ]
    got = {name: call() for name, call, _ in cases}
    assert got == {name: code for name, _, code in cases}
    assert not buf.any()


def test_no_device_is_an_error_not_a_fallback():
    import torch
    if torch.cuda.is_available():
        return   # with a device the same calls are the GPU tests' business
    from lambda_elliptic_curves_amd import _lib
    L = C.CDLL(_lib.LIB_PATH)
    a, b = np.arange(16, dtype=np.uint32), np.zeros(16, np.uint32)
    pa, pb = C.c_void_p(a.ctypes.data), C.c_void_p(b.ctypes.data)
    u32, sz = C.c_uint32, C.c_size_t
    assert L.lw_circle_evaluate_cfft(pa, pb, u32(4), u32(1), sz(0)) == _lib.ERR_NO_DEVICE
    assert L.lw_circle_interpolate_cfft(pa, pb, u32(4), u32(1), sz(0)) == _lib.ERR_NO_DEVICE
    assert L.lw_circle_get_twiddles(u32(4), C.c_int(0), pb) == _lib.ERR_NO_DEVICE
    assert not b.any()


def test_wrapper_errors_and_empty_interpolate():
    from lambda_elliptic_curves_amd import circle, errors
    for bad in (np.ones(3, np.uint32), np.ones(1, np.uint32), np.ones((2, 6), np.uint32), np.ones(0, np.uint32)):
        with pytest.raises(errors.InputError):
            circle.evaluate_cfft(bad)
    for bad in (np.ones(3, np.uint32), np.ones(1, np.uint32), np.ones((2, 12), np.uint32)):
        with pytest.raises(errors.InputError):
            circle.interpolate_cfft(bad)
    out = circle.interpolate_cfft(np.empty(0, np.uint32))
    assert out.shape == (0,) and out.dtype == np.uint32
    with pytest.raises(errors.OrderError):
        circle.get_twiddles(31, circle.TWIDDLES_EVALUATION)
    with pytest.raises(errors.HipError):
        circle.get_twiddles(0, circle.TWIDDLES_EVALUATION)
