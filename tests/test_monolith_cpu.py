"""Monolith over Mersenne31 without a device: the restatement the GPU tests compare against (tests/monolith_ref.py)
against the reference's three recorded vectors, the generated constants against their rule, the permutation header
compiled for the host and run under sanitizers (tests/monolith_host_main.cpp), and the boundary (exports, status codes,
wrapper errors) of the new entry points."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

from tests import monolith_ref as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = M.P
SYMBOLS = ["lw_monolith_permute", "lw_monolith_permute_device", "lw_monolith_hash", "lw_monolith_hash_device", "lw_monolith_compress",
           "lw_monolith_compress_device", "lw_monolith_commit_columns", "lw_monolith_commit_columns_device", "lw_monolith_constants",
           "lw_monolith_layer_device"]


def golden():
    with open(os.path.join(ROOT, "tests", "golden", "monolith_mersenne31.json")) as f:
        return json.load(f)


# ---- 1. the restatement against the reference's recorded vectors
def test_restatement_reproduces_the_three_vectors():
    g = golden()
    for name in ("from_plonky3_concrete_width_16", "from_plonky3_concrete_width_12"):
        w, r = g[name]["width"], g[name]["rounds"]
        assert M.concrete(list(range(w)), M.constants(w, r)[1]) == g[name]["expected"], name
        assert M.np_concrete(np.arange(w, dtype=np.uint64).reshape(1, w), M.constants(w, r)[1])[0].tolist() == g[name]["expected"], name
    v = g["from_plonky3_width_16"]
    assert (v["width"], v["rounds"]) == (16, 5)
    assert M.permute(16, 5, list(range(16))) == v["expected"]


def test_parameters_and_bounds():
    assert sum(M.CIRC16) == 524757 and max(M.CIRC16) < 1 << 16 and sum(M.CIRC16) * P < 1 << 51   # the accumulator of monolith.cuh
    assert 4 * P * P < 1 << 64                                                                   # four Cauchy products in a u64
    assert M.bar(0) == 0 and M.bar(P) == P                                                       # both spellings of zero agree
    assert sorted(M.s_box(y) for y in range(256)) == list(range(256))
    assert sorted(M.final_s_box(y) for y in range(128)) == list(range(128))
    for w, r in ((8, 1), (12, 5), (20, 3), (24, 15)):
        rc, mds = M.constants(w, r)
        assert len(rc) == r and all(len(row) == w and all(0 <= c < P for c in row) for row in rc)
        assert len(mds) == w and all(len(row) == w and all(0 < m < P for m in row) for row in mds)
    assert M.constants(16, 5)[1][1][:3] == [M.CIRC16[15], M.CIRC16[0], M.CIRC16[1]]              # rotated right


# ---- 2. the numpy form against the integer form
def test_numpy_form_is_the_integer_form():
    rng = np.random.default_rng(3)
    for w, r in ((8, 1), (12, 5), (16, 5), (20, 2), (24, 15)):
        s = np.concatenate([np.array(M.edge_states(w), np.uint32), rng.integers(0, 1 << 32, (3, w), dtype=np.uint32)])
        out = M.np_permute(w, r, s)
        assert out.dtype == np.uint32 and (out < P).all()
        assert out.tolist() == [M.permute(w, r, [int(v) for v in row]) for row in s]
    for length in (0, 1, 7, 8, 9, 16, 17):
        rows = rng.integers(0, 1 << 32, (2, length), dtype=np.uint32)
        assert M.np_hash(5, rows).tolist() == [M.hash(5, [int(v) for v in row]) for row in rows], length
    assert not M.np_hash(5, np.zeros((3, 0), np.uint32)).any()
    assert M.hash(5, [7]) == M.hash(5, [7, 0])   # no padding: what the docstrings warn about
    left, right = rng.integers(0, 1 << 32, (3, 8), dtype=np.uint32), rng.integers(0, 1 << 32, (3, 8), dtype=np.uint32)
    assert M.np_compress(5, left, right).tolist() == [M.compress(5, [int(v) for v in a], [int(v) for v in b]) for a, b in zip(left, right)]
    cols = rng.integers(0, 1 << 32, (3, 4), dtype=np.uint32)   # a tree of 4 leaves by hand
    for br in (False, True):
        nodes = M.np_tree(5, cols, br)
        order = [0, 2, 1, 3] if br else [0, 1, 2, 3]
        leaves = [M.hash(5, [int(cols[c, j]) for c in range(3)]) for j in order]
        l01, l23 = M.compress(5, leaves[0], leaves[1]), M.compress(5, leaves[2], leaves[3])
        assert nodes.tolist() == [M.compress(5, l01, l23), l01, l23] + leaves


# ---- 3. the generated constants
@pytest.mark.parametrize("width,rounds", [(16, 5), (12, 5), (8, 1), (24, 15)])
def test_constants_follow_their_rule(width, rounds):
    from lambda_elliptic_curves_amd import monolith
    rc, mds = monolith.constants(width, rounds)
    exp_rc, exp_mds = M.constants(width, rounds)
    assert rc.dtype == np.uint32 and rc.tolist() == exp_rc
    assert mds.tolist() == exp_mds


# ---- 4. the permutation header on the host, under AddressSanitizer and UndefinedBehaviorSanitizer.  monolith.cuh is plain
# C++ for the host and the device alike, so the program runs the very source the kernels compile.
@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    hipcc = "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        hipcc = "hipcc"
    exe = tmp_path_factory.mktemp("monolith") / "monolith_host_main"
    subprocess.check_call([hipcc, "-x", "hip", "--cuda-host-only", "-O2", "-std=c++17", "-Xarch_host", "-fsanitize=address,undefined",
                           "-Xarch_host", "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "lambda_elliptic_curves_amd", "csrc"),
                           os.path.join(ROOT, "tests", "monolith_host_main.cpp"), "-o", str(exe)], timeout=600)

    def run(text):
        out = subprocess.run([str(exe)], input=text, capture_output=True, text=True, timeout=120)
        assert out.returncode == 0, out.stderr
        return out.stdout.split("\n")[:-1]
    return run


def test_swar_bars_is_the_table_definition(host_program):
    words = M.bars_words()
    assert len(words) == 7 + 2 * (3 * 256 + 128)
    rng = np.random.default_rng(11)
    words += [int(v) for v in rng.integers(0, 1 << 31, 2000)]
    lines = host_program("B %d %s\n" % (len(words), " ".join(str(w) for w in words)))
    assert lines == ["B %d" % M.bar(w) for w in words]
    assert M.bar(0x00FFFFFF) == 0x00FFFFFF and M.bar(1) == 2


def test_host_program_permutes_like_the_restatement(host_program):
    rng = np.random.default_rng(12)
    text, want = [], []
    flat = lambda rows: " ".join(str(int(v)) for row in rows for v in row)
    for w, r in ((8, 1), (8, 5), (12, 5), (16, 5), (16, 15), (20, 5), (24, 5), (24, 15)):
        rc, mds = M.constants(w, r)
        states = M.edge_states(w) + rng.integers(0, 1 << 32, (4, w), dtype=np.uint32).tolist()
        text.append("P %d %d %d %s %s %s" % (w, r, len(states), flat(rc), flat(mds), flat(states)))
        want += ["P " + " ".join(str(v) for v in M.permute(w, r, st)) for st in states]
    for w in (16, 24):   # Concrete alone on the largest accumulators
        mds = M.constants(w, 5)[1]
        states = [[P] * w, [0xFFFFFFFF] * w, [P - 1] * w]
        text.append("L %d 0 %d %s %s" % (w, len(states), flat(mds), flat(states)))
        want += ["L " + " ".join(str(v) for v in M.concrete([M.reduce_word(x) for x in st], mds)) for st in states]
    text.append("L 12 2 1 %s %s" % (flat(M.constants(12, 5)[1]), flat([[P] * 12])))   # Bricks with all words p
    want.append("L " + " ".join(["0"] * 12))
    assert host_program("\n".join(text) + "\n") == want
    g = golden()["from_plonky3_width_16"]["expected"]   # the recorded vector through the header itself
    rc, mds = M.constants(16, 5)
    assert host_program("P 16 5 1 %s %s %s\n" % (flat(rc), flat(mds), " ".join(str(v) for v in range(16)))) == ["P " + " ".join(str(v) for v in g)]


# ---- 5. the boundary
def test_symbols_are_exported_and_declared():
    from lambda_elliptic_curves_amd import _lib
    L = _lib.lib()
    header = open(os.path.join(ROOT, "include", "lw_hip.h")).read()
    ffi = open(os.path.join(ROOT, "rust-shim", "src", "ffi.rs")).read()
    for sym in SYMBOLS:
        assert sym in _lib.EXPORTS and hasattr(L, sym)
        assert getattr(L, sym).argtypes is not None
        assert sym + "(" in header and "pub fn " + sym + "(" in ffi
    assert "typedef enum { LW_MONOLITH_CONCRETE = 0, LW_MONOLITH_BARS = 1, LW_MONOLITH_BRICKS = 2 } lw_monolith_layer_t;" in header
    for name, val in (("CONCRETE", 0), ("BARS", 1), ("BRICKS", 2)):
        assert "pub const LW_MONOLITH_%s: c_int = %d;" % (name, val) in ffi
    shim = open(os.path.join(ROOT, "rust-shim", "src", "lib.rs")).read()
    for fn in ("monolith_permute_hip", "monolith_hash_hip", "monolith_compress_hip", "monolith_commit_columns_hip"):
        assert "pub fn %s(" % fn in shim
    import lambda_elliptic_curves_amd as pkg
    assert "monolith" in pkg.__all__
    assert (pkg.monolith.LAYER_CONCRETE, pkg.monolith.LAYER_BARS, pkg.monolith.LAYER_BRICKS) == (0, 1, 2)
    for fn in ("permute", "hash", "compress", "commit_columns", "constants", "permute_device", "hash_device", "compress_device",
               "commit_columns_device", "layer_device"):
        assert callable(getattr(pkg.monolith, fn))


# ---- 6. every bad argument returns its code without a device
def test_status_codes_need_no_device():
    from lambda_elliptic_curves_amd import _lib
    L = C.CDLL(_lib.LIB_PATH)   # a handle of its own: plain ctypes arguments, no argtypes
    buf = np.zeros(1 << 12, np.uint64)
    assert buf.ctypes.data % 16 == 0
    at = lambda words: C.c_void_p(buf.ctypes.data + 4 * words)
    A, B, D, ODD, N = at(0), at(4096), at(2048), at(1), C.c_void_p(None)
    i, u32, u64, sz = C.c_int, C.c_uint32, C.c_uint64, C.c_size_t
    BAD, ALLOC, OK = _lib.ERR_BAD_ARG, _lib.ERR_ALLOC, _lib.OK
    W, R = u32(16), u32(5)
    cases = [
        # no work: nothing touched, null buffers included
        ("permute n=0", lambda: L.lw_monolith_permute(W, R, N, sz(0), N), OK),
        ("permute_device n=0", lambda: L.lw_monolith_permute_device(W, R, N, sz(0), N, N), OK),
        ("layer_device n=0", lambda: L.lw_monolith_layer_device(W, R, i(1), N, sz(0), N, N), OK),
        ("hash n_rows=0", lambda: L.lw_monolith_hash(R, N, sz(0), sz(3), N), OK),
        ("hash_device n_rows=0", lambda: L.lw_monolith_hash_device(R, N, sz(0), sz(3), sz(0), N, N), OK),
        ("compress n=0", lambda: L.lw_monolith_compress(R, N, N, sz(0), N), OK),
        ("compress_device n=0", lambda: L.lw_monolith_compress_device(R, N, N, sz(0), N, N), OK),
        # null pointers
        ("permute null in", lambda: L.lw_monolith_permute(W, R, N, sz(1), B), BAD),
        ("permute null out", lambda: L.lw_monolith_permute(W, R, A, sz(1), N), BAD),
        ("permute_device null", lambda: L.lw_monolith_permute_device(W, R, N, sz(1), B, N), BAD),
        ("layer_device null", lambda: L.lw_monolith_layer_device(W, R, i(0), A, sz(1), N, N), BAD),
        ("hash null rows", lambda: L.lw_monolith_hash(R, N, sz(1), sz(2), B), BAD),
        ("hash null out", lambda: L.lw_monolith_hash(R, A, sz(1), sz(0), N), BAD),
        ("hash_device null rows", lambda: L.lw_monolith_hash_device(R, N, sz(1), sz(2), sz(0), B, N), BAD),
        ("hash_device null out", lambda: L.lw_monolith_hash_device(R, A, sz(1), sz(2), sz(0), N, N), BAD),
        ("compress null left", lambda: L.lw_monolith_compress(R, N, D, sz(1), B), BAD),
        ("compress null right", lambda: L.lw_monolith_compress(R, A, N, sz(1), B), BAD),
        ("compress null out", lambda: L.lw_monolith_compress(R, A, D, sz(1), N), BAD),
        ("compress_device null", lambda: L.lw_monolith_compress_device(R, A, N, sz(1), B, N), BAD),
        ("commit null columns", lambda: L.lw_monolith_commit_columns(R, N, u32(1), u32(2), i(0), B, N), BAD),
        ("commit null root", lambda: L.lw_monolith_commit_columns(R, A, u32(1), u32(2), i(0), N, N), BAD),
        ("commit_device null nodes", lambda: L.lw_monolith_commit_columns_device(R, A, u32(1), u64(0), u32(2), i(0), N, N, N), BAD),
        ("commit_device null columns", lambda: L.lw_monolith_commit_columns_device(R, N, u32(1), u64(0), u32(2), i(0), B, N, N), BAD),
        ("commit no columns", lambda: L.lw_monolith_commit_columns(R, A, u32(0), u32(2), i(0), B, N), BAD),
        ("commit_device no columns", lambda: L.lw_monolith_commit_columns_device(R, A, u32(0), u64(0), u32(2), i(0), B, N, N), BAD),
        ("constants null rc", lambda: L.lw_monolith_constants(W, R, N, B), BAD),
        ("constants null mds", lambda: L.lw_monolith_constants(W, R, A, N), BAD),
        # device buffers that are not 16-byte aligned
        ("permute_device misaligned in", lambda: L.lw_monolith_permute_device(W, R, ODD, sz(1), B, N), BAD),
        ("permute_device misaligned out", lambda: L.lw_monolith_permute_device(W, R, A, sz(1), ODD, N), BAD),
        ("layer_device misaligned", lambda: L.lw_monolith_layer_device(W, R, i(0), ODD, sz(1), B, N), BAD),
        ("hash_device misaligned", lambda: L.lw_monolith_hash_device(R, ODD, sz(1), sz(2), sz(0), B, N), BAD),
        ("compress_device misaligned", lambda: L.lw_monolith_compress_device(R, A, ODD, sz(1), B, N), BAD),
        ("commit_device misaligned columns", lambda: L.lw_monolith_commit_columns_device(R, ODD, u32(1), u64(0), u32(2), i(0), B, N, N), BAD),
        ("commit_device misaligned nodes", lambda: L.lw_monolith_commit_columns_device(R, A, u32(1), u64(0), u32(2), i(0), ODD, N, N), BAD),
        # strides below the length
        ("hash_device row stride", lambda: L.lw_monolith_hash_device(R, A, sz(2), sz(5), sz(4), B, N), BAD),
        ("commit_device column stride", lambda: L.lw_monolith_commit_columns_device(R, A, u32(2), u64(3), u32(2), i(0), B, N, N), BAD),
        # a layer that does not exist
        ("layer_device layer 3", lambda: L.lw_monolith_layer_device(W, R, i(3), A, sz(1), B, N), BAD),
        ("layer_device layer -1", lambda: L.lw_monolith_layer_device(W, R, i(-1), A, sz(1), B, N), BAD),
        # sizes past what can be addressed: the bounds of lw_rpo_*
        ("commit 2^31 leaves", lambda: L.lw_monolith_commit_columns(R, A, u32(1), u32(31), i(0), B, N), ALLOC),
        ("commit_device 2^31 leaves", lambda: L.lw_monolith_commit_columns_device(R, A, u32(1), u64(0), u32(31), i(0), B, N, N), ALLOC),
        ("permute 2^36 + 1", lambda: L.lw_monolith_permute(W, R, A, sz((1 << 36) + 1), B), ALLOC),
        ("compress 2^36 + 1", lambda: L.lw_monolith_compress(R, A, D, sz((1 << 36) + 1), B), ALLOC),
        ("hash row_len 2^31 + 1", lambda: L.lw_monolith_hash(R, A, sz(1), sz((1 << 31) + 1), B), ALLOC),
    ]
    for bad in (0, 4, 7, 10, 17, 28, 32):
        V = u32(bad)
        tag = " width %d" % bad
        cases += [
            ("permute" + tag, lambda V=V: L.lw_monolith_permute(V, R, A, sz(1), B), BAD),
            ("permute n=0" + tag, lambda V=V: L.lw_monolith_permute(V, R, N, sz(0), N), BAD),
            ("permute_device" + tag, lambda V=V: L.lw_monolith_permute_device(V, R, A, sz(1), B, N), BAD),
            ("layer_device" + tag, lambda V=V: L.lw_monolith_layer_device(V, R, i(0), A, sz(1), B, N), BAD),
            ("constants" + tag, lambda V=V: L.lw_monolith_constants(V, R, A, B), BAD),
        ]
    for bad in (0, 16, 255, 0xFFFFFFFF):
        V = u32(bad)
        tag = " rounds %d" % bad
        cases += [
            ("permute" + tag, lambda V=V: L.lw_monolith_permute(W, V, A, sz(1), B), BAD),
            ("permute_device" + tag, lambda V=V: L.lw_monolith_permute_device(W, V, A, sz(1), B, N), BAD),
            ("layer_device" + tag, lambda V=V: L.lw_monolith_layer_device(W, V, i(0), A, sz(1), B, N), BAD),
            ("hash" + tag, lambda V=V: L.lw_monolith_hash(V, A, sz(1), sz(2), B), BAD),
            ("hash n_rows=0" + tag, lambda V=V: L.lw_monolith_hash(V, N, sz(0), sz(2), N), BAD),
            ("hash_device" + tag, lambda V=V: L.lw_monolith_hash_device(V, A, sz(1), sz(2), sz(0), B, N), BAD),
            ("compress" + tag, lambda V=V: L.lw_monolith_compress(V, A, D, sz(1), B), BAD),
            ("compress_device" + tag, lambda V=V: L.lw_monolith_compress_device(V, A, D, sz(1), B, N), BAD),
            ("commit" + tag, lambda V=V: L.lw_monolith_commit_columns(V, A, u32(1), u32(2), i(0), B, N), BAD),
            ("commit_device" + tag, lambda V=V: L.lw_monolith_commit_columns_device(V, A, u32(1), u64(0), u32(2), i(0), B, N, N), BAD),
            ("constants" + tag, lambda V=V: L.lw_monolith_constants(W, V, A, B), BAD),
        ]
    got = {name: call() for name, call, _ in cases}
    assert got == {name: code for name, _, code in cases}
    assert len(got) == len(cases) and not buf.any()


# ---- 7. no device: an error, not a fallback
def test_host_forms_fail_loudly_without_a_device():
    import torch
    from lambda_elliptic_curves_amd import errors, monolith
    if not torch.cuda.is_available():
        with pytest.raises(errors.HipError):
            monolith.permute(16, 5, np.zeros((1, 16), np.uint32))
        with pytest.raises(errors.HipError):
            monolith.permute(24, 5, np.zeros((1, 24), np.uint32))
        with pytest.raises(errors.HipError):
            monolith.hash(5, np.arange(3, dtype=np.uint32))
        with pytest.raises(errors.HipError):
            monolith.compress(5, np.zeros((1, 8), np.uint32), np.ones((1, 8), np.uint32))
        with pytest.raises(errors.HipError):
            monolith.commit_columns(5, np.zeros((2, 4), np.uint32))
    assert monolith.permute(12, 5, np.zeros((0, 12), np.uint32)).shape == (0, 12)   # no work: no device needed
    assert monolith.hash(5, np.zeros((0, 5), np.uint32)).shape == (0, 8)
    assert monolith.compress(5, np.zeros((0, 8), np.uint32), np.zeros((0, 8), np.uint32)).shape == (0, 8)
    with pytest.raises(errors.InputError):
        monolith.commit_columns(5, np.zeros((2, 3), np.uint32))
    for bad in ((10, 5), (16, 0), (16, 16)):
        with pytest.raises(ValueError):
            monolith.permute(bad[0], bad[1], np.zeros((1, 16), np.uint32))
        with pytest.raises(ValueError):
            monolith.constants(*bad)
    with pytest.raises(ValueError):
        monolith.hash(0, np.zeros(3, np.uint32))
    assert (monolith.P, monolith.DIGEST_LEN, monolith.RATE, monolith.SPONGE_WIDTH, monolith.WIDTHS) == (P, 8, 8, 16, M.WIDTHS)
