"""The BabyBear quartic extension without a device: the arithmetic header compiled for the host and run under sanitizers
against Python integers, four properties of the model the GPU tests compare against (tests/babybear_ext_ref.py), and the
argument checks of the new entry points, which all run before any device work."""
import ctypes as C
import os
import subprocess

import numpy as np

from tests import babybear_ext_ref as X

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = X.P
SYMBOLS = ["lw_babybear_ext4_pointwise_device", "lw_babybear_ext4_convert_device", "lw_babybear_ext4_evaluate_device",
           "lw_babybear_ext4_deep_quotients_device", "lw_babybear_ext4_fri_layer_device"]


def grid4(words):
    """words^4 as (4, len^4) uint64 planes, the first component outermost"""
    w = np.array(words, np.uint64)
    return np.stack([g.reshape(-1) for g in np.meshgrid(w, w, w, w, indexing="ij")])


# ---- the arithmetic header on the host, sanitised, as a child process
def test_host_program_of_the_arithmetic_header(tmp_path):
    hipcc = "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        hipcc = "hipcc"
    exe = tmp_path / "babybear_ext_host"
    subprocess.check_call([hipcc, "-x", "hip", "--cuda-host-only", "-O2", "-std=c++17", "-Xarch_host", "-fsanitize=address,undefined",
                           "-Xarch_host", "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "lambda_elliptic_curves_amd", "csrc"),
                           os.path.join(ROOT, "tests", "babybear_ext_host_main.cpp"), "-o", str(exe)], timeout=600)
    E, B = X.EDGE, X.EDGE_B
    assert len(E) == 8 and P - 1 in E and P - 1 in B
    out = subprocess.run([str(exe), str(len(E))] + [str(v) for v in E + B], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    got = np.array(out.stdout.split(), dtype=np.uint64).reshape(-1, 4)   # decimal words, four to a line
    ea, ba = grid4(E), grid4(B)                      # stored words
    ua, ub = X.np_unstore(ea), X.np_unstore(ba)      # the residues they stand for
    na, nb = ea.shape[1], ba.shape[1]
    assert (na, nb) == (4096, 256)
    # mul: E^4 x B^4, the all-(p - 1) pair among them
    want = X.np_store(X.np_mul(np.repeat(ua, nb, axis=1), np.tile(ub, (1, na)))).T
    assert np.array_equal(got[:na * nb], want)
    k = na * nb
    # spot check in Python integers: a = (E[3], E[3], E[3], E[3]) and b = (B[2], B[2], B[2], B[2]), all p - 1
    ia = sum(3 * 8 ** t for t in range(4))
    ib = sum(2 * 4 ** t for t in range(4))
    a, b = X.unstore_elem(ea[:, ia]), X.unstore_elem(ba[:, ib])
    assert ea[:, ia].tolist() == [P - 1] * 4 and ba[:, ib].tolist() == [P - 1] * 4
    assert got[ia * nb + ib].tolist() == list(X.store_elem(X.mul(a, b)))
    # sqr, inv, a inv(a)
    elems = X.elems_of(ua)
    want = []
    for a in elems:
        v = X.inv(a)
        one = X.mul(a, v)
        assert one == (X.ONE if a != X.ZERO else X.ZERO)          # a inv(a) = 1 for every non-zero a, inv(0) = 0
        want += [X.store_elem(X.sqr(a)), X.store_elem(v), X.store_elem(one)]
    assert got[k:k + 3 * na].tolist() == [list(w) for w in want]
    k += 3 * na
    # mul_base: E^4 x E
    ue = X.np_unstore(np.array(E, np.uint64))
    want = X.np_store(X.np_mul_base(np.repeat(ua, len(E), axis=1), np.tile(ue, na))).T
    assert np.array_equal(got[k:k + na * len(E)], want)
    k += na * len(E)
    # add, sub, neg on neighbouring edge words
    for i in range(len(E)):
        a = X.unstore_elem([E[(i + t) % 8] for t in range(4)])
        b = X.unstore_elem([E[(i + 4 + t) % 8] for t in range(4)])
        assert got[k:k + 3].tolist() == [list(X.store_elem(X.add(a, b))), list(X.store_elem(X.sub(a, b))), list(X.store_elem(X.sub(X.ZERO, a)))]
        k += 3
    assert got[k:].tolist() == [list(X.store_elem((P - 11, 0, 0, 0))), [0, 0, 0, 0]]      # x^4 = -11, inv(0) = 0


# ---- the model
def rand_elems(n, seed):
    return [tuple(int(v) for v in row) for row in np.random.default_rng(seed).integers(0, P, (n, 4))]


def test_model_field_has_inverses_and_mul_is_schoolbook_reduction_by_x4_equals_minus_11():
    """x^4 + 11 has no root and no quadratic factor over F_p exactly when every non-zero element has an inverse: a inv(a) = 1
    over the edges and 10^3 random elements."""
    edge = [X.unstore_elem(e) for e in X.elems_of(grid4(X.EDGE)[:, ::7])]
    elems = edge + rand_elems(1000, 31)
    for a in elems:
        if a != X.ZERO:
            assert X.mul(a, X.inv(a)) == X.ONE
    assert X.inv(X.ZERO) == X.ZERO
    for a, b in zip(elems[:300], elems[::-1][:300]):
        # the schoolbook product, seven coefficients, then x^4 -> -11 from the top down
        c = [0] * 7
        for i in range(4):
            for j in range(4):
                c[i + j] += a[i] * b[j]
        for d in (6, 5, 4):
            c[d - 4] -= X.BETA * c[d]
        assert X.mul(a, b) == tuple(v % P for v in c[:4])
        assert X.sqr(a) == X.mul(a, a) and X.power(a, 5) == X.mul(X.sqr(X.sqr(a)), a)
        assert X.mul_base(a, b[0]) == X.mul(a, (b[0], 0, 0, 0))
    pa, pb = X.planes_of(elems), X.planes_of(elems[::-1])
    assert X.elems_of(X.np_mul(pa, pb)) == [X.mul(a, b) for a, b in zip(elems, elems[::-1])]
    assert X.elems_of(X.np_mul_base(pa, pb[2])) == [X.mul_base(a, b[2]) for a, b in zip(elems, elems[::-1])]
    col = np.random.default_rng(35).integers(0, P, 2500).astype(np.uint64)
    assert X.np_horner(col, elems[40]) == X.horner(col.tolist(), elems[40]) and X.np_horner(col[:5], elems[41], 4) == X.horner(col[:5].tolist(), elems[41])
    words = np.array(X.EDGE + [12345], np.uint64)
    assert X.np_store(X.np_unstore(words)).tolist() == words.tolist() == [X.store(X.unstore(w)) for w in words.tolist()]


def test_model_fold_satisfies_the_verifiers_identity():
    """e'[i] = (a + b) + zeta (a - b) / x_i with a = e[i], b = e[i + N/2] = p(-x_i), e' on the squared coset."""
    N, h = 64, 7
    coeffs = rand_elems(13, 32)
    zeta = rand_elems(1, 33)[0]
    e = X.layer_evaluation(coeffs + [X.ZERO] * 3, N, h)
    assert e == X.elems_of(X.np_layer_evaluation(coeffs + [X.ZERO] * 3, N, h))
    block = X.fold(coeffs, zeta)
    assert len(block) == 8 and block[7] == X.ZERO
    e2 = X.layer_evaluation(block, N // 2, h * h % P)
    w = X.root_of_unity(6)
    assert pow(w, 32, P) == P - 1
    for i in range(N // 2):
        a, b = e[i], e[i + N // 2]
        x_inv = pow(h * pow(w, i, P) % P, P - 2, P)
        assert e2[i] == X.add(X.add(a, b), X.mul(zeta, X.mul_base(X.sub(a, b), x_inv)))
    assert e[5] == X.horner_ext(coeffs, (h * pow(w, 5, P) % P, 0, 0, 0))


def test_model_pair_rule_is_the_chunks_of_the_bit_reversed_vector():
    for L in range(1, 8):
        n = 1 << L
        br = [X.bitrev(i, L) for i in range(n)]   # in_place_bit_reverse_permute: position k holds e[bitrev(k)]
        for j in range(n // 2):
            i = X.pair_index(j, n)
            assert (br[2 * j], br[2 * j + 1]) == (i, i + n // 2)
    planes = np.arange(32, dtype=np.uint64).reshape(4, 8)
    assert X.layer_rows(planes).tolist() == [[0, 8, 16, 24, 4, 12, 20, 28], [2, 10, 18, 26, 6, 14, 22, 30], [1, 9, 17, 25, 5, 13, 21, 29],
                                             [3, 11, 19, 27, 7, 15, 23, 31]]
    # the tree over those rows from the definition: 32-byte leaves of big-endian stored words, 2-to-1 nodes, root first
    for n in (2, 8):
        planes = np.random.default_rng(34).integers(0, P, (4, n)).astype(np.uint64)
        rows = X.np_store(X.layer_rows(planes))
        level = [X.leaf_hash(r) for r in rows]
        levels = [level]
        while len(level) > 1:
            level = [X.O.keccak256(level[2 * k] + level[2 * k + 1]) for k in range(len(level) // 2)]
            levels.append(level)
        assert X.layer_tree(planes).tobytes() == b"".join(b"".join(lv) for lv in reversed(levels))


# ---- the boundary
def test_symbols_are_exported_and_declared():
    from lambda_elliptic_curves_amd import _lib, babybear_ext
    L = _lib.lib()
    header = open(os.path.join(ROOT, "include", "lw_hip.h")).read()
    ffi = open(os.path.join(ROOT, "rust-shim", "src", "ffi.rs")).read()
    for sym in SYMBOLS:
        assert sym in _lib.EXPORTS and hasattr(L, sym)
        assert sym + "(" in header and "pub fn " + sym + "(" in ffi
    a, b = (3, 5, 7, 9), (2, 4, 6, 8)
    assert babybear_ext.times_x(X.store_elem(a)) == X.store_elem(X.mul((0, 1, 0, 0), a))
    vals = [X.store_elem(v) for v in (a, b, (1, 0, 0, 2), (0, 0, 5, 0))]
    want = X.ZERO
    for e, v in enumerate(vals):
        want = X.add(want, X.mul(X.power((0, 1, 0, 0), e), X.unstore_elem(v)))
    assert babybear_ext.combine_planes(vals) == X.store_elem(want)
    rows = babybear_ext.plane_weights([X.store_elem(a), X.store_elem(b)])
    assert rows == [[X.store_elem(X.mul(X.power((0, 1, 0, 0), e), w)) for w in (a, b)] for e in range(4)]
    assert [babybear_ext.folded_block(n) for n in (1, 2, 3, 5, 513, 4096)] == [X.folded_block(n) for n in (1, 2, 3, 5, 513, 4096)] == [2, 2, 2, 4, 512, 2048]
    assert [babybear_ext.to_mont(v) for v in (0, 1, P - 1, 12345)] == [X.store(v) for v in (0, 1, P - 1, 12345)]
    assert [babybear_ext.from_mont(babybear_ext.to_mont(v)) for v in (0, 1, P - 1, 12345)] == [0, 1, P - 1, 12345]


def test_status_codes_need_no_device():
    from lambda_elliptic_curves_amd import _lib
    L = C.CDLL(_lib.LIB_PATH)   # a handle of its own: plain ctypes arguments, no argtypes
    raw = np.zeros((1 << 13) + 4, np.uint32)
    base = (raw.ctypes.data + 15) & ~15
    at = lambda words: C.c_void_p(base + 4 * words)
    A, B, O, N = at(0), at(2048), at(4096), C.c_void_p(None)
    u32, sz, i = C.c_uint32, C.c_size_t, C.c_int
    OK, BAD, POW2, ROOTERR, ZERO = _lib.OK, _lib.ERR_BAD_ARG, _lib.ERR_INPUT_NOT_POW2, _lib.ERR_ROOT_OF_UNITY, _lib.ERR_INV_ZERO
    words = lambda *v: (C.c_uint32 * len(v))(*v)
    zero, pword, seven = words(0), words(P), words(7)
    pts, base_pt, p_pt = words(3, 5, 9, 11, 1, 0, 0, 2), words(3, 5, 9, 11, 4, 0, 0, 0), words(3, 5, P, 11, 1, 0, 0, 2)
    tab = words(*range(1, 25))   # 3 columns x 2 points
    p_tab = words(*(list(range(1, 24)) + [P]))
    values = words(*([99] * 24))
    MUL, SQR, INV, MULB = 0, 1, 2, 3
    pw = lambda op, a, sa, b, sb, out, so, n: L.lw_babybear_ext4_pointwise_device(i(op), a, sz(sa), b, sz(sb), out, sz(so), sz(n), N)
    cv = lambda d, inter, planes, stride, n: L.lw_babybear_ext4_convert_device(i(d), inter, planes, sz(stride), sz(n), N)
    ev = lambda d, k, stride, n, p, m, out: L.lw_babybear_ext4_evaluate_device(d, u32(k), sz(stride), sz(n), p, u32(m), out, N)
    dq = lambda d, k, stride, lg, off, p, m, w, e, out, so: L.lw_babybear_ext4_deep_quotients_device(
        d, u32(k), sz(stride), u32(lg), off, p, u32(m), w, e, out, sz(so), N)
    fl = lambda d, stride, n, z, off, dom, poly, evl, nodes, rt=N: L.lw_babybear_ext4_fri_layer_device(
        d, sz(stride), sz(n), z, off, sz(dom), poly, evl, nodes, rt, N)
    E, T = at(6144), at(7168)   # evaluation and nodes of a layer
    cases = [
        ("pointwise null a", lambda: pw(MUL, N, 0, B, 0, O, 0, 16), BAD),
        ("pointwise null b", lambda: pw(MUL, A, 0, N, 0, O, 0, 16), BAD),
        ("pointwise null base b", lambda: pw(MULB, A, 0, N, 0, O, 0, 16), BAD),
        ("pointwise null out", lambda: pw(SQR, A, 0, N, 0, N, 0, 16), BAD),
        ("pointwise misaligned a", lambda: pw(INV, at(1), 0, N, 0, O, 0, 16), BAD),
        ("pointwise misaligned out", lambda: pw(INV, A, 0, N, 0, at(4097), 0, 16), BAD),
        ("pointwise a stride", lambda: pw(MUL, A, 15, B, 0, O, 0, 16), BAD),
        ("pointwise b stride", lambda: pw(MUL, A, 0, B, 15, O, 0, 16), BAD),
        ("pointwise out stride", lambda: pw(MUL, A, 0, B, 0, O, 15, 16), BAD),
        ("pointwise overlap a", lambda: pw(SQR, A, 0, N, 0, at(8), 0, 16), BAD),
        ("pointwise overlap a's last plane", lambda: pw(SQR, A, 0, N, 0, at(60), 0, 16), BAD),
        ("pointwise overlap b", lambda: pw(MUL, A, 0, B, 0, at(2048 + 24), 0, 16), BAD),
        ("pointwise overlap base b", lambda: pw(MULB, A, 0, B, 0, at(2048 - 48 - 8), 0, 16), BAD),
        ("pointwise out is base b", lambda: pw(MULB, A, 0, B, 0, B, 0, 16), BAD),
        ("pointwise in place, other stride", lambda: pw(SQR, A, 16, N, 0, A, 64, 16), BAD),
        ("pointwise op 4", lambda: pw(4, A, 0, B, 0, O, 0, 16), BAD),
        ("pointwise op -1", lambda: pw(-1, A, 0, B, 0, O, 0, 16), BAD),
        ("pointwise n 0", lambda: pw(MUL, N, 0, N, 0, N, 0, 0), OK),
        ("convert null interleaved", lambda: cv(0, N, O, 0, 16), BAD),
        ("convert null planes", lambda: cv(1, A, N, 0, 16), BAD),
        ("convert misaligned", lambda: cv(0, at(1), O, 0, 16), BAD),
        ("convert stride", lambda: cv(0, A, O, 15, 16), BAD),
        ("convert overlap", lambda: cv(0, A, at(124), 0, 16), BAD),
        ("convert direction 2", lambda: cv(2, A, O, 0, 16), BAD),
        ("convert n 0", lambda: cv(0, N, N, 0, 0), OK),
        ("evaluate null coefficients", lambda: ev(N, 3, 0, 16, pts, 2, values), BAD),
        ("evaluate null points", lambda: ev(A, 3, 0, 16, N, 2, values), BAD),
        ("evaluate null values", lambda: ev(A, 3, 0, 16, pts, 2, N), BAD),
        ("evaluate misaligned", lambda: ev(at(1), 3, 0, 16, pts, 2, values), BAD),
        ("evaluate stride", lambda: ev(A, 3, 15, 16, pts, 2, values), BAD),
        ("evaluate point word p", lambda: ev(A, 3, 0, 16, p_pt, 2, values), BAD),
        ("evaluate no points", lambda: ev(N, 3, 0, 16, N, 0, N), OK),
        ("deep null columns", lambda: dq(N, 3, 0, 4, N, pts, 2, tab, tab, O, 0), BAD),
        ("deep null out", lambda: dq(A, 3, 0, 4, N, pts, 2, tab, tab, N, 0), BAD),
        ("deep null points", lambda: dq(A, 3, 0, 4, N, N, 2, tab, tab, O, 0), BAD),
        ("deep null weights", lambda: dq(A, 3, 0, 4, N, pts, 2, N, tab, O, 0), BAD),
        ("deep null evals", lambda: dq(A, 3, 0, 4, N, pts, 2, tab, N, O, 0), BAD),
        ("deep no columns", lambda: dq(A, 0, 0, 4, N, pts, 2, tab, tab, O, 0), BAD),
        ("deep no points", lambda: dq(A, 3, 0, 4, N, pts, 0, tab, tab, O, 0), BAD),
        ("deep misaligned", lambda: dq(A, 3, 0, 4, N, pts, 2, tab, tab, at(4097), 0), BAD),
        ("deep column stride", lambda: dq(A, 3, 15, 4, N, pts, 2, tab, tab, O, 0), BAD),
        ("deep out stride", lambda: dq(A, 3, 0, 4, N, pts, 2, tab, tab, O, 15), BAD),
        ("deep overlap", lambda: dq(A, 3, 0, 4, N, pts, 2, tab, tab, at(40), 0), BAD),
        ("deep base-field point", lambda: dq(A, 3, 0, 4, N, base_pt, 2, tab, tab, O, 0), BAD),
        ("deep point word p", lambda: dq(A, 3, 0, 4, N, p_pt, 2, tab, tab, O, 0), BAD),
        ("deep weight word p", lambda: dq(A, 3, 0, 4, N, pts, 2, p_tab, tab, O, 0), BAD),
        ("deep eval word p", lambda: dq(A, 3, 0, 4, N, pts, 2, tab, p_tab, O, 0), BAD),
        ("deep log2n 25", lambda: dq(A, 3, 0, 25, N, pts, 2, tab, tab, O, 0), ROOTERR),
        ("deep offset 0", lambda: dq(A, 3, 0, 4, zero, pts, 2, tab, tab, O, 0), ZERO),
        ("deep offset p", lambda: dq(A, 3, 0, 4, pword, pts, 2, tab, tab, O, 0), BAD),
        ("layer null coefficients", lambda: fl(N, 0, 16, pts, seven, 32, O, E, T), BAD),
        ("layer null zeta", lambda: fl(A, 0, 16, N, seven, 32, O, E, T), BAD),
        ("layer zeta word p", lambda: fl(A, 0, 16, words(1, 2, 3, P), seven, 32, O, E, T), BAD),
        ("layer null poly", lambda: fl(A, 0, 16, pts, seven, 32, N, E, T), BAD),
        ("layer misaligned coefficients", lambda: fl(at(1), 0, 16, pts, seven, 32, O, E, T), BAD),
        ("layer misaligned nodes", lambda: fl(A, 0, 16, pts, seven, 32, O, E, at(7169)), BAD),
        ("layer stride", lambda: fl(A, 15, 16, pts, seven, 32, O, E, T), BAD),
        ("layer poly overlaps coefficients", lambda: fl(A, 0, 16, pts, seven, 32, at(60), E, T), BAD),
        ("layer evaluation overlaps poly", lambda: fl(A, 0, 16, pts, seven, 32, O, at(4096 + 28), T), BAD),
        ("layer nodes overlap evaluation", lambda: fl(A, 0, 16, pts, seven, 32, O, E, at(6144 + 124)), BAD),
        ("layer domain 6", lambda: fl(A, 0, 4, pts, seven, 6, O, E, T), POW2),
        ("layer domain 0", lambda: fl(A, 0, 4, pts, seven, 0, O, E, T), POW2),
        ("layer domain 2^25", lambda: fl(A, 0, 4, pts, seven, 1 << 25, O, E, T), ROOTERR),
        ("layer domain below the block", lambda: fl(A, 0, 16, pts, seven, 4, O, E, T), BAD),
        ("layer nodes without evaluation", lambda: fl(A, 0, 16, pts, seven, 32, O, N, T), BAD),
        ("layer evaluation without nodes", lambda: fl(A, 0, 16, pts, seven, 32, O, E, N), BAD),
        ("layer root without nodes", lambda: fl(A, 0, 16, pts, seven, 32, O, N, N, values), BAD),
        ("layer offset 0", lambda: fl(A, 0, 16, pts, zero, 32, O, E, T), ZERO),
        ("layer n 0", lambda: fl(N, 0, 0, N, N, 0, N, N, N), OK),
    ]
    got = {name: call() for name, call, _ in cases}
    assert got == {name: code for name, _, code in cases}
    assert not raw.any() and list(values) == [99] * 24 and list(pts) == [3, 5, 9, 11, 1, 0, 0, 2] and seven[0] == 7
    # the zero polynomial needs no device either: zeros to the host
    assert ev(A, 3, 0, 0, pts, 2, values) == OK and list(values) == [0] * 24


def test_no_device_is_an_error_not_a_fallback():
    import torch
    if torch.cuda.is_available():
        return   # with a device the same calls are the GPU tests' business
    from lambda_elliptic_curves_amd import _lib
    L = C.CDLL(_lib.LIB_PATH)
    raw = np.zeros(1 << 11, np.uint32)
    base = (raw.ctypes.data + 15) & ~15
    at = lambda w: C.c_void_p(base + 4 * w)
    N = C.c_void_p(None)
    u32, sz, i = C.c_uint32, C.c_size_t, C.c_int
    pts = (C.c_uint32 * 4)(3, 5, 7, 9)
    out = (C.c_uint32 * 4)(9, 9, 9, 9)
    assert L.lw_babybear_ext4_pointwise_device(i(1), at(0), sz(0), N, sz(0), at(256), sz(0), sz(8), N) == _lib.ERR_NO_DEVICE
    assert L.lw_babybear_ext4_convert_device(i(0), at(0), at(256), sz(0), sz(8), N) == _lib.ERR_NO_DEVICE
    assert L.lw_babybear_ext4_evaluate_device(at(0), u32(1), sz(0), sz(8), pts, u32(1), out, N) == _lib.ERR_NO_DEVICE
    assert L.lw_babybear_ext4_deep_quotients_device(at(0), u32(1), sz(0), u32(3), N, pts, u32(1), pts, pts, at(256), sz(0), N) == _lib.ERR_NO_DEVICE
    assert L.lw_babybear_ext4_fri_layer_device(at(0), sz(0), sz(8), pts, N, sz(0), at(256), N, N, N, N) == _lib.ERR_NO_DEVICE
    assert not raw.any() and list(out) == [9, 9, 9, 9]
