"""The Goldilocks quadratic extension without a device: the arithmetic header compiled for the host and run under
sanitizers against Python integers, three properties of the model the GPU tests compare against
(tests/goldilocks_ext_ref.py), and the argument checks of the new entry points, which all run before any device work."""
import ctypes as C
import os
import subprocess

import numpy as np

from tests import goldilocks_ext_ref as X
from tests import goldilocks_ref as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = G.P
SYMBOLS = ["lw_goldilocks_ext2_pointwise_device", "lw_goldilocks_ext2_evaluate_device", "lw_goldilocks_ext2_deep_quotients_device",
           "lw_goldilocks_ext2_fri_layer_device"]


# ---- the arithmetic header on the host, sanitised, as a child process
def test_host_program_of_the_arithmetic_header(tmp_path):
    hipcc = "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        hipcc = "hipcc"
    exe = tmp_path / "goldilocks_ext_host"
    subprocess.check_call([hipcc, "-x", "hip", "--cuda-host-only", "-O2", "-std=c++17", "-Xarch_host", "-fsanitize=address,undefined",
                           "-Xarch_host", "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "lambda_elliptic_curves_amd", "csrc"),
                           os.path.join(ROOT, "tests", "goldilocks_ext_host_main.cpp"), "-o", str(exe)], timeout=600)
    out = subprocess.run([str(exe)] + [str(v) for v in G.EDGE], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    E = G.EDGE
    want = []
    for a0 in E:
        for a1 in E:
            a = (a0, a1)
            row0 = [(a0 * b0 + 7 * a1 * b1) % P for b0 in E for b1 in E]
            row1 = [(a0 * b1 + a1 * b0) % P for b0 in E for b1 in E]
            want += ["m %d %d" % r for r in zip(row0, row1)]
            v = X.inv(a)
            one = X.mul(a, v)
            assert one == ((1, 0) if a != (0, 0) else (0, 0))          # a inv(a) = 1 for every non-zero a, inv(0) = 0
            want.append("s %d %d %d %d %d %d" % (X.sqr(a) + v + one))
            want += ["b %d %d" % X.mul_base(a, b) for b in E]
    for i in range(len(E) - 3):
        a, b = (E[i], E[i + 1]), (E[i + 2], E[i + 3])
        want.append("x %d %d %d %d %d %d" % (X.add(a, b) + X.sub(a, b) + X.sub((0, 0), a)))
    want.append("z 0 0 %d 0 0 %d" % (P - 1, (1 << 64) - 1 - P))
    got = out.stdout.split("\n")
    assert len(E) ** 4 + len(E) ** 2 + len(E) ** 3 == sum(1 for w in want if w[0] in "msb") == 614656 + 784 + 21952
    assert got[:len(want)] == want and got[len(want):] == [""]


# ---- the model
def test_model_mul_is_schoolbook_reduction_by_t2_equals_7():
    assert pow(7, (P - 1) // 2, P) == P - 1   # 7 is a non-residue: t^2 - 7 is irreducible
    rng = np.random.default_rng(31)
    pairs = [tuple(int(v) % P for v in rng.integers(0, 1 << 64, 2, dtype=np.uint64)) for _ in range(64)]
    pairs += [(a, b) for a in G.EDGE[::3] for b in G.EDGE[1::4]]
    for a in pairs[:40]:
        for b in pairs[40:]:
            # (a0 + a1 t)(b0 + b1 t) = a0 b0 + (a0 b1 + a1 b0) t + a1 b1 t^2, then t^2 -> 7
            c = [a[0] * b[0], a[0] * b[1] + a[1] * b[0], a[1] * b[1]]
            assert X.mul(a, b) == ((c[0] + 7 * c[2]) % P, c[1] % P)
        if a != (0, 0):
            assert X.mul(a, X.inv(a)) == (1, 0)
        assert X.sqr(a) == X.mul(a, a) and X.power(a, 5) == X.mul(X.sqr(X.sqr(a)), a)
    a0 = np.array([p[0] for p in pairs], np.uint64)
    a1 = np.array([p[1] for p in pairs], np.uint64)
    r0, r1 = X.np_mul(a0, a1, a1[::-1].copy(), a0[::-1].copy())
    assert list(zip(r0.tolist(), r1.tolist())) == [X.mul(p, (q[1], q[0])) for p, q in zip(pairs, pairs[::-1])]


def test_model_fold_satisfies_the_verifiers_identity():
    """e'[i] = (a + b) + zeta (a - b) / x_i with a = e[i], b = e[i + N/2] = p(-x_i), e' on the squared coset."""
    rng = np.random.default_rng(32)
    N, h = 64, 7
    coeffs = [tuple(int(v) % P for v in rng.integers(0, 1 << 64, 2, dtype=np.uint64)) for _ in range(13)]
    zeta = (int(rng.integers(1, 1 << 62)), int(rng.integers(1, 1 << 62)))
    e = X.layer_evaluation(coeffs + [X.ZERO] * 3, N, h)
    assert e == [tuple(int(v) for v in col) for col in X.np_layer_evaluation(coeffs + [X.ZERO] * 3, N, h).T]
    block = X.fold(coeffs, zeta)
    assert len(block) == 8 and block[7] == X.ZERO
    e2 = X.layer_evaluation(block, N // 2, h * h % P)
    w = G.root_of_unity(6)
    for i in range(N // 2):
        a, b = e[i], e[i + N // 2]
        x_inv = pow(h * pow(w, i, P) % P, P - 2, P)
        assert e2[i] == X.add(X.add(a, b), X.mul(zeta, X.mul_base(X.sub(a, b), x_inv)))
    assert e[5] == X.horner_ext(coeffs, (h * pow(w, 5, P) % P, 0))


def test_model_pair_rule_is_the_chunks_of_the_bit_reversed_vector():
    for L in range(1, 8):
        n = 1 << L
        br = [G.bitrev(i, L) for i in range(n)]   # in_place_bit_reverse_permute: position k holds e[bitrev(k)]
        for j in range(n // 2):
            i = X.pair_index(j, n)
            assert (br[2 * j], br[2 * j + 1]) == (i, i + n // 2)
    planes = np.arange(16, dtype=np.uint64).reshape(2, 8)
    assert X.layer_rows(planes).tolist() == [[0, 8, 4, 12], [2, 10, 6, 14], [1, 9, 5, 13], [3, 11, 7, 15]]


# ---- the boundary
def test_symbols_are_exported_and_declared():
    from lambda_elliptic_curves_amd import _lib, goldilocks_ext
    L = _lib.lib()
    header = open(os.path.join(ROOT, "include", "lw_hip.h")).read()
    ffi = open(os.path.join(ROOT, "rust-shim", "src", "ffi.rs")).read()
    for sym in SYMBOLS:
        assert sym in _lib.EXPORTS and hasattr(L, sym)
        assert sym + "(" in header and "pub fn " + sym + "(" in ffi
    assert goldilocks_ext.times_t((3, 5)) == X.mul((0, 1), (3, 5))
    assert goldilocks_ext.combine_planes((1, 2), (3, 4)) == X.add((1, 2), X.mul((0, 1), (3, 4)))
    assert [goldilocks_ext.folded_block(n) for n in (1, 2, 3, 5, 513, 4096)] == [X.folded_block(n) for n in (1, 2, 3, 5, 513, 4096)] == [2, 2, 2, 4, 512, 2048]


def test_status_codes_need_no_device():
    from lambda_elliptic_curves_amd import _lib
    L = C.CDLL(_lib.LIB_PATH)   # a handle of its own: plain ctypes arguments, no argtypes
    raw = np.zeros((1 << 12) + 2, np.uint64)
    base = (raw.ctypes.data + 15) & ~15
    at = lambda words: C.c_void_p(base + 8 * words)
    A, B, O, N = at(0), at(1024), at(2048), C.c_void_p(None)
    u32, u64, sz, i = C.c_uint32, C.c_uint64, C.c_size_t, C.c_int
    OK, BAD, POW2, ORDER, ROOTERR, ZERO = (_lib.OK, _lib.ERR_BAD_ARG, _lib.ERR_INPUT_NOT_POW2, _lib.ERR_ORDER_TOO_LARGE, _lib.ERR_ROOT_OF_UNITY,
                                           _lib.ERR_INV_ZERO)
    words = lambda *v: (C.c_uint64 * len(v))(*v)
    zero, pword, seven = words(0), words(P), words(7)
    pts, base_pt, p_pt = words(3, 5, 9, 11), words(3, 5, 9, 0), words(3, P, 9, 11)
    tab = words(*range(1, 13))   # 3 columns x 2 points
    values = words(*([99] * 12))
    MUL, SQR, INV, MULB = 0, 1, 2, 3
    pw = lambda op, a, sa, b, sb, out, so, n: L.lw_goldilocks_ext2_pointwise_device(i(op), a, sz(sa), b, sz(sb), out, sz(so), sz(n), N)
    ev = lambda d, k, stride, n, p, m, out: L.lw_goldilocks_ext2_evaluate_device(d, u32(k), sz(stride), sz(n), p, u32(m), out, N)
    dq = lambda d, k, stride, lg, off, root, p, m, w, e, out, so: L.lw_goldilocks_ext2_deep_quotients_device(
        d, u32(k), sz(stride), u32(lg), off, u64(root), p, u32(m), w, e, out, sz(so), N)
    fl = lambda d, stride, n, z, off, dom, root, level, poly, evl, nodes, rt=N: L.lw_goldilocks_ext2_fri_layer_device(
        d, sz(stride), sz(n), z, off, sz(dom), u64(root), i(level), poly, evl, nodes, rt, N)
    E, T = at(3072), at(3584)   # evaluation and nodes of a layer
    cases = [
        ("pointwise null a", lambda: pw(MUL, N, 0, B, 0, O, 0, 16), BAD),
        ("pointwise null b", lambda: pw(MUL, A, 0, N, 0, O, 0, 16), BAD),
        ("pointwise null base b", lambda: pw(MULB, A, 0, N, 0, O, 0, 16), BAD),
        ("pointwise null out", lambda: pw(SQR, A, 0, N, 0, N, 0, 16), BAD),
        ("pointwise misaligned a", lambda: pw(INV, at(1), 0, N, 0, O, 0, 16), BAD),
        ("pointwise misaligned out", lambda: pw(INV, A, 0, N, 0, at(2049), 0, 16), BAD),
        ("pointwise a stride", lambda: pw(MUL, A, 15, B, 0, O, 0, 16), BAD),
        ("pointwise b stride", lambda: pw(MUL, A, 0, B, 15, O, 0, 16), BAD),
        ("pointwise out stride", lambda: pw(MUL, A, 0, B, 0, O, 15, 16), BAD),
        ("pointwise overlap a", lambda: pw(SQR, A, 0, N, 0, at(8), 0, 16), BAD),
        ("pointwise overlap b", lambda: pw(MUL, A, 0, B, 0, at(1024 + 24), 0, 16), BAD),
        ("pointwise overlap base b", lambda: pw(MULB, A, 0, B, 0, at(1024 - 16 - 8), 0, 16), BAD),
        ("pointwise in place, other stride", lambda: pw(SQR, A, 16, N, 0, A, 64, 16), BAD),
        ("pointwise out is a's other plane", lambda: pw(SQR, A, 16, N, 0, at(16), 16, 16), BAD),
        ("pointwise op 4", lambda: pw(4, A, 0, B, 0, O, 0, 16), BAD),
        ("pointwise op -1", lambda: pw(-1, A, 0, B, 0, O, 0, 16), BAD),
        ("pointwise n 0", lambda: pw(MUL, N, 0, N, 0, N, 0, 0), OK),
        ("evaluate null coefficients", lambda: ev(N, 3, 0, 16, pts, 2, values), BAD),
        ("evaluate null points", lambda: ev(A, 3, 0, 16, N, 2, values), BAD),
        ("evaluate null values", lambda: ev(A, 3, 0, 16, pts, 2, N), BAD),
        ("evaluate misaligned", lambda: ev(at(1), 3, 0, 16, pts, 2, values), BAD),
        ("evaluate stride", lambda: ev(A, 3, 15, 16, pts, 2, values), BAD),
        ("evaluate no points", lambda: ev(N, 3, 0, 16, N, 0, N), OK),
        ("deep null columns", lambda: dq(N, 3, 0, 4, N, 0, pts, 2, tab, tab, O, 0), BAD),
        ("deep null out", lambda: dq(A, 3, 0, 4, N, 0, pts, 2, tab, tab, N, 0), BAD),
        ("deep null points", lambda: dq(A, 3, 0, 4, N, 0, N, 2, tab, tab, O, 0), BAD),
        ("deep null weights", lambda: dq(A, 3, 0, 4, N, 0, pts, 2, N, tab, O, 0), BAD),
        ("deep null evals", lambda: dq(A, 3, 0, 4, N, 0, pts, 2, tab, N, O, 0), BAD),
        ("deep no columns", lambda: dq(A, 0, 0, 4, N, 0, pts, 2, tab, tab, O, 0), BAD),
        ("deep misaligned", lambda: dq(A, 3, 0, 4, N, 0, pts, 2, tab, tab, at(2049), 0), BAD),
        ("deep column stride", lambda: dq(A, 3, 15, 4, N, 0, pts, 2, tab, tab, O, 0), BAD),
        ("deep out stride", lambda: dq(A, 3, 0, 4, N, 0, pts, 2, tab, tab, O, 15), BAD),
        ("deep overlap", lambda: dq(A, 3, 0, 4, N, 0, pts, 2, tab, tab, at(40), 0), BAD),
        ("deep base-field point", lambda: dq(A, 3, 0, 4, N, 0, base_pt, 2, tab, tab, O, 0), BAD),
        ("deep point with c1 = p", lambda: dq(A, 3, 0, 4, N, 0, p_pt, 2, tab, tab, O, 0), BAD),
        ("deep log2n 31", lambda: dq(A, 3, 0, 31, N, 0, pts, 2, tab, tab, O, 0), ORDER),
        ("deep log2n 33", lambda: dq(A, 3, 0, 33, N, 0, pts, 2, tab, tab, O, 0), ROOTERR),
        ("deep root of order 4", lambda: dq(A, 3, 0, 4, N, 1 << 48, pts, 2, tab, tab, O, 0), ROOTERR),
        ("deep offset 0", lambda: dq(A, 3, 0, 4, zero, 0, pts, 2, tab, tab, O, 0), ZERO),
        ("deep offset p", lambda: dq(A, 3, 0, 4, pword, 0, pts, 2, tab, tab, O, 0), ZERO),
        ("layer null coefficients", lambda: fl(N, 0, 16, pts, seven, 32, 0, 0, O, E, T), BAD),
        ("layer null zeta", lambda: fl(A, 0, 16, N, seven, 32, 0, 0, O, E, T), BAD),
        ("layer null poly", lambda: fl(A, 0, 16, pts, seven, 32, 0, 0, N, E, T), BAD),
        ("layer misaligned coefficients", lambda: fl(at(1), 0, 16, pts, seven, 32, 0, 0, O, E, T), BAD),
        ("layer misaligned nodes", lambda: fl(A, 0, 16, pts, seven, 32, 0, 0, O, E, at(3585)), BAD),
        ("layer stride", lambda: fl(A, 15, 16, pts, seven, 32, 0, 0, O, E, T), BAD),
        ("layer poly overlaps coefficients", lambda: fl(A, 0, 16, pts, seven, 32, 0, 0, at(24), E, T), BAD),
        ("layer evaluation overlaps poly", lambda: fl(A, 0, 16, pts, seven, 32, 0, 0, O, at(2048 + 8), T), BAD),
        ("layer level 2", lambda: fl(A, 0, 16, pts, seven, 32, 0, 2, O, E, T), BAD),
        ("layer level 2, fold only", lambda: fl(A, 0, 16, pts, N, 0, 0, 2, O, N, N), BAD),
        ("layer domain 6", lambda: fl(A, 0, 4, pts, seven, 6, 0, 0, O, E, T), POW2),
        ("layer domain 0", lambda: fl(A, 0, 4, pts, seven, 0, 0, 0, O, E, T), POW2),
        ("layer domain below the block", lambda: fl(A, 0, 16, pts, seven, 4, 0, 0, O, E, T), BAD),
        ("layer nodes without evaluation", lambda: fl(A, 0, 16, pts, seven, 32, 0, 0, O, N, T), BAD),
        ("layer evaluation without nodes", lambda: fl(A, 0, 16, pts, seven, 32, 0, 0, O, E, N), BAD),
        ("layer root without nodes", lambda: fl(A, 0, 16, pts, seven, 32, 0, 0, O, N, N, values), BAD),
        ("layer offset 0", lambda: fl(A, 0, 16, pts, zero, 32, 0, 0, O, E, T), ZERO),
        ("layer root of order 4", lambda: fl(A, 0, 16, pts, seven, 32, 1 << 48, 0, O, E, T), ROOTERR),
        ("layer n 0", lambda: fl(N, 0, 0, N, N, 0, 0, 0, N, N, N), OK),
    ]
    got = {name: call() for name, call, _ in cases}
    assert got == {name: code for name, _, code in cases}
    assert not raw.any() and list(values) == [99] * 12 and list(pts) == [3, 5, 9, 11] and seven[0] == 7
    # the zero polynomial needs no device either: zeros to the host
    assert ev(A, 3, 0, 0, pts, 2, values) == OK and list(values) == [0] * 12


def test_no_device_is_an_error_not_a_fallback():
    import torch
    if torch.cuda.is_available():
        return   # with a device the same calls are the GPU tests' business
    from lambda_elliptic_curves_amd import _lib
    L = C.CDLL(_lib.LIB_PATH)
    raw = np.zeros(1 << 10, np.uint64)
    base = (raw.ctypes.data + 15) & ~15
    at = lambda w: C.c_void_p(base + 8 * w)
    N = C.c_void_p(None)
    u32, u64, sz, i = C.c_uint32, C.c_uint64, C.c_size_t, C.c_int
    pts = (C.c_uint64 * 2)(3, 5)
    out = (C.c_uint64 * 2)(9, 9)
    assert L.lw_goldilocks_ext2_pointwise_device(i(1), at(0), sz(0), N, sz(0), at(64), sz(0), sz(8), N) == _lib.ERR_NO_DEVICE
    assert L.lw_goldilocks_ext2_evaluate_device(at(0), u32(1), sz(0), sz(8), pts, u32(1), out, N) == _lib.ERR_NO_DEVICE
    assert L.lw_goldilocks_ext2_deep_quotients_device(at(0), u32(1), sz(0), u32(3), N, u64(0), pts, u32(1), pts, pts, at(64), sz(0), N) == _lib.ERR_NO_DEVICE
    assert L.lw_goldilocks_ext2_fri_layer_device(at(0), sz(0), sz(8), pts, N, sz(0), u64(0), i(0), at(64), N, N, N, N) == _lib.ERR_NO_DEVICE
    assert not raw.any() and list(out) == [9, 9]
