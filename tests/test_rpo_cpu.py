"""Rescue Prime Optimized without a device: the restatement the GPU tests compare against (tests/rpo_ref.py) against the
reference's 38 fixed digests, the generated round constants against their rule, the permutation header compiled for the
host and run under sanitizers, and the boundary (exports, status codes, wrapper errors) of the new entry points."""
import ctypes as C
import hashlib
import json
import os
import re
import subprocess

import numpy as np
import pytest

from tests import goldilocks_ref as G
from tests import rpo_ref as R
from tools import gen_rpo_consts as GEN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = R.P
LEVELS = (R.LEVEL_128, R.LEVEL_160)
SYMBOLS = ["lw_rpo_permute", "lw_rpo_permute_device", "lw_rpo_hash", "lw_rpo_hash_device", "lw_rpo_commit_columns",
           "lw_rpo_commit_columns_device"]


def golden():
    with open(os.path.join(ROOT, "tests", "golden", "rpo_goldilocks.json")) as f:
        g = json.load(f)
    return {R.LEVEL_128: [[int(x) for x in row] for row in g["EXPECTED_128"]],
            R.LEVEL_160: [[int(x) for x in row] for row in g["EXPECTED_160"]]}


# ---- 1. the restatement against the reference's fixed digests: digest i = hash([0, 1, .., i])
def test_restatement_reproduces_the_38_digests():
    g = golden()
    assert len(g[R.LEVEL_128]) == 19 and len(g[R.LEVEL_160]) == 19
    for level in LEVELS:
        for i, exp in enumerate(g[level]):
            assert len(exp) == R.digest_len(level)
            assert R.hash(level, list(range(i + 1))) == exp, (level, i)


def test_parameters():
    assert R.ALPHA * R.ALPHA_INV % (P - 1) == 1
    for level, (sec, m, cap, v) in R.PARAMS.items():
        assert len(v) == m and len(R.RC[level]) == 2 * m * 7 and all(0 <= c < P for c in R.RC[level])
    assert sum(R.PARAMS[R.LEVEL_128][3]) == 160                      # the MDS bounds of rpo.cuh
    assert sum(R.PARAMS[R.LEVEL_160][3]) == 1363684766 < 1 << 31
    assert all(x & (x - 1) == 0 for x in R.PARAMS[R.LEVEL_160][3])   # shifts
    for x in G.EDGE:
        assert R.sbox_inv_chain(x) == pow(x, R.ALPHA_INV, P) and pow(R.sbox_inv_chain(x), 7, P) == x


# ---- 2. the numpy form against the integer form
def test_numpy_form_is_the_integer_form():
    rng = np.random.default_rng(3)
    for level in LEVELS:
        m, rt = R.width(level), R.rate(level)
        s = np.array(R.edge_states(level)[:8] + R.edge_states(level)[-3:], np.uint64)
        s = np.concatenate([s, rng.integers(0, 1 << 64, (3, m), dtype=np.uint64)])
        out = R.np_permute(level, s)
        assert out.tolist() == [R.permute(level, [int(v) for v in row]) for row in s]
        assert (out < np.uint64(P)).all()
        assert R.np_mds(level, G.np_reduce(s)).tolist() == [R.mds(level, [int(v) % P for v in row]) for row in s]
        for length in (0, 1, rt - 1, rt, rt + 1, 2 * rt, 2 * rt + 1):
            rows = rng.integers(0, 1 << 64, (2, length), dtype=np.uint64)
            assert R.np_hash(level, rows).tolist() == [R.hash(level, [int(v) for v in row]) for row in rows], length
        assert not R.np_hash(level, np.zeros((3, 0), np.uint64)).any()
    # a tree of 4 leaves by hand
    cols = rng.integers(0, 1 << 64, (3, 4), dtype=np.uint64)
    for level in LEVELS:
        for br in (False, True):
            nodes = R.np_tree(level, cols, br)
            order = [0, 2, 1, 3] if br else [0, 1, 2, 3]
            leaves = [R.hash(level, [int(cols[c, j]) for c in range(3)]) for j in order]
            l01, l23 = R.hash(level, leaves[0] + leaves[1]), R.hash(level, leaves[2] + leaves[3])
            assert nodes.tolist() == [R.hash(level, l01 + l23), l01, l23] + leaves


# ---- 3. the committed constants
def test_rpo_consts_inc_matches_generator():
    with open(GEN.output_path()) as f:
        committed = f.read()
    assert GEN.render() == committed, "rpo_consts.inc is stale: run python3 tools/gen_rpo_consts.py"


def test_committed_constants_follow_the_shake256_rule():
    # parsed from the committed file and compared with the rule spelled out here once more
    with open(GEN.output_path()) as f:
        text = f.read()
    for sec, m, cap in ((128, 12, 4), (160, 16, 6)):
        block = re.search(r"#ifdef RPO_CONSTS_%d\n(.*?)#endif" % sec, text, re.S).group(1)
        words = [int(w, 16) for w in re.findall(r"0x([0-9a-f]{16})ull,", block)]
        assert len(words) == 2 * m * 7
        stream = hashlib.shake_256(("RPO(%d,%d,%d,%d)" % (P, m, cap, sec)).encode()).digest(9 * len(words))
        for i, w in enumerate(words):
            assert w < P and w == int.from_bytes(stream[9 * i:9 * i + 9], "little") % P, (sec, i)
        assert words == R.RC[R.LEVEL_128 if sec == 128 else R.LEVEL_160]


# ---- 4. the permutation header on the host.  rpo.cuh is plain C++ for the host and the device alike (no inline
# assembly), so the twin runs the very source the kernels compile; the GPU tests run the device's code object.
TWIN = r"""
#include <stdio.h>
#include <inttypes.h>
#include "rpo.cuh"
using namespace lw;
static const uint64_t edge[] = {%(edge)s};
static const uint64_t states0[] = {%(states0)s};
static const uint64_t states1[] = {%(states1)s};
template <int LEVEL> static void digests() {   // hash([0 .. i]), i < 19: the sponge of rescue_prime_optimized.rs:205-230
    typedef RpoParams<LEVEL> R;
    for (int len = 1; len <= 19; len++) {
        uint64_t s[R::M] = {0};
        if (len %% R::RATE) s[0] = 1;
        for (int b = 0; b < (len + R::RATE - 1) / R::RATE; b++) {
            for (int h = 0; h < R::RATE; h++) {
                const int c = b * R::RATE + h;
                s[R::CAP + h] = c < len ? (uint64_t)c : (c == len ? 1 : 0);
            }
            rpo_permute<LEVEL>(s);
        }
        printf("d%%d", LEVEL);
        for (int j = 0; j < R::DIGEST; j++) printf(" %%" PRIu64, s[R::CAP + j]);
        printf("\n");
    }
}
template <int LEVEL> static void permutations(const uint64_t *states, int n) {
    constexpr int M = RpoParams<LEVEL>::M;
    for (int i = 0; i < n; i++) {
        uint64_t s[M];
        for (int j = 0; j < M; j++) s[j] = gl_from_word(states[i * M + j]);
        rpo_permute<LEVEL>(s);
        printf("p%%d", LEVEL);
        for (int j = 0; j < M; j++) printf(" %%" PRIu64, s[j]);
        printf("\n");
    }
}
int main() {
    digests<0>();
    digests<1>();
    permutations<0>(states0, sizeof(states0) / sizeof(states0[0]) / 12);
    permutations<1>(states1, sizeof(states1) / sizeof(states1[0]) / 16);
    const int n = sizeof(edge) / sizeof(edge[0]);
    for (int i = 0; i < n; i += 4) {   // the S-box chains on every EDGE operand, four side by side
        uint64_t a[4], b[4];
        for (int j = 0; j < 4; j++) a[j] = b[j] = edge[i + j < n ? i + j : n - 1];
        rpo_sbox<4>(a);
        rpo_sbox_inv<4>(b);
        for (int j = 0; j < 4; j++) printf("s %%" PRIu64 " %%" PRIu64 "\n", a[j], b[j]);
    }
    uint64_t m0[12], m1[16];   // the MDS on non-canonical words: the largest half-sums
    for (int j = 0; j < 12; j++) m0[j] = 0xFFFFFFFFFFFFFFFFull;
    for (int j = 0; j < 16; j++) m1[j] = 0xFFFFFFFFFFFFFFFFull;
    rpo_mds<0>(m0);
    rpo_mds<1>(m1);
    printf("m %%" PRIu64 " %%" PRIu64 "\n", m0[5], m1[7]);
    return 0;
}
"""


def test_host_twin_of_the_permutation_header(tmp_path):
    hipcc = "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        hipcc = "hipcc"
    flat = lambda states: ", ".join("%dull" % w for st in states for w in st)
    src = tmp_path / "twin.cpp"
    src.write_text(TWIN % {"edge": ", ".join("%dull" % v for v in G.EDGE), "states0": flat(R.edge_states(R.LEVEL_128)),
                           "states1": flat(R.edge_states(R.LEVEL_160))})
    exe = tmp_path / "twin"
    subprocess.check_call([hipcc, "-x", "hip", "--cuda-host-only", "-O2", "-std=c++17", "-Xarch_host", "-fsanitize=address,undefined",
                           "-Xarch_host", "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "lambda_elliptic_curves_amd", "csrc"),
                           str(src), "-o", str(exe)], timeout=600)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    lines = out.stdout.split("\n")
    g = golden()
    want = []
    for level in LEVELS:
        want += ["d%d %s" % (level, " ".join(str(v) for v in row)) for row in g[level]]
    for level in LEVELS:
        want += ["p%d %s" % (level, " ".join(str(v) for v in R.permute(level, st))) for st in R.edge_states(level)]
    padded = G.EDGE + [G.EDGE[-1]] * (-len(G.EDGE) % 4)
    want += ["s %d %d" % (pow(x, 7, P), pow(x, R.ALPHA_INV, P)) for x in padded]
    full = (1 << 64) - 1
    want += ["m %d %d" % (160 * full % P, 1363684766 * full % P)]
    assert lines[:len(want)] == want
    assert len(want) == 38 + 2 * 60 + 28 + 1


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
    assert "typedef enum { LW_RPO_128 = 0, LW_RPO_160 = 1 } lw_rpo_level_t;" in header
    assert "pub const LW_RPO_128: c_int = 0;" in ffi and "pub const LW_RPO_160: c_int = 1;" in ffi
    shim = open(os.path.join(ROOT, "rust-shim", "src", "lib.rs")).read()
    assert "pub fn rpo_permute_hip(" in shim and "pub fn rpo_hash_hip(" in shim and "pub fn rpo_commit_columns_hip(" in shim
    import lambda_elliptic_curves_amd as pkg
    assert pkg.rpo.LEVEL_128 == _lib.RPO_128 == 0 and pkg.rpo.LEVEL_160 == _lib.RPO_160 == 1 and "rpo" in pkg.__all__


# ---- 6. every bad argument returns its code without a device
def test_status_codes_need_no_device():
    from lambda_elliptic_curves_amd import _lib
    L = C.CDLL(_lib.LIB_PATH)   # a handle of its own: plain ctypes arguments, no argtypes
    buf = np.zeros(1 << 12, np.uint64)
    assert buf.ctypes.data % 16 == 0
    at = lambda words: C.c_void_p(buf.ctypes.data + 8 * words)
    A, B, ODD, N = at(0), at(2048), at(1), C.c_void_p(None)
    i, u32, u64, sz = C.c_int, C.c_uint32, C.c_uint64, C.c_size_t
    BAD, ALLOC, OK = _lib.ERR_BAD_ARG, _lib.ERR_ALLOC, _lib.OK
    cases = []
    for lv in (0, 1):
        V = i(lv)
        tag = " level %d" % lv
        cases += [
            # no work: nothing touched, null buffers included
            ("permute n=0" + tag, lambda V=V: L.lw_rpo_permute(V, N, sz(0), N), OK),
            ("permute_device n=0" + tag, lambda V=V: L.lw_rpo_permute_device(V, N, sz(0), N, N), OK),
            ("hash n_rows=0" + tag, lambda V=V: L.lw_rpo_hash(V, N, sz(0), sz(3), N), OK),
            ("hash_device n_rows=0" + tag, lambda V=V: L.lw_rpo_hash_device(V, N, sz(0), sz(3), sz(0), N, N), OK),
            # null pointers
            ("permute null in" + tag, lambda V=V: L.lw_rpo_permute(V, N, sz(1), B), BAD),
            ("permute null out" + tag, lambda V=V: L.lw_rpo_permute(V, A, sz(1), N), BAD),
            ("permute_device null" + tag, lambda V=V: L.lw_rpo_permute_device(V, N, sz(1), B, N), BAD),
            ("hash null rows" + tag, lambda V=V: L.lw_rpo_hash(V, N, sz(1), sz(2), B), BAD),
            ("hash null out" + tag, lambda V=V: L.lw_rpo_hash(V, A, sz(1), sz(0), N), BAD),
            ("hash_device null rows" + tag, lambda V=V: L.lw_rpo_hash_device(V, N, sz(1), sz(2), sz(0), B, N), BAD),
            ("hash_device null out" + tag, lambda V=V: L.lw_rpo_hash_device(V, A, sz(1), sz(2), sz(0), N, N), BAD),
            ("commit null columns" + tag, lambda V=V: L.lw_rpo_commit_columns(V, N, u32(1), u32(2), i(0), B, N), BAD),
            ("commit null root" + tag, lambda V=V: L.lw_rpo_commit_columns(V, A, u32(1), u32(2), i(0), N, N), BAD),
            ("commit_device null nodes" + tag, lambda V=V: L.lw_rpo_commit_columns_device(V, A, u32(1), u64(0), u32(2), i(0), N, N, N), BAD),
            ("commit_device null columns" + tag, lambda V=V: L.lw_rpo_commit_columns_device(V, N, u32(1), u64(0), u32(2), i(0), B, N, N), BAD),
            ("commit no columns" + tag, lambda V=V: L.lw_rpo_commit_columns(V, A, u32(0), u32(2), i(0), B, N), BAD),
            ("commit_device no columns" + tag, lambda V=V: L.lw_rpo_commit_columns_device(V, A, u32(0), u64(0), u32(2), i(0), B, N, N), BAD),
            # device buffers that are not 16-byte aligned
            ("permute_device misaligned in" + tag, lambda V=V: L.lw_rpo_permute_device(V, ODD, sz(1), B, N), BAD),
            ("permute_device misaligned out" + tag, lambda V=V: L.lw_rpo_permute_device(V, A, sz(1), ODD, N), BAD),
            ("hash_device misaligned" + tag, lambda V=V: L.lw_rpo_hash_device(V, ODD, sz(1), sz(2), sz(0), B, N), BAD),
            ("commit_device misaligned columns" + tag, lambda V=V: L.lw_rpo_commit_columns_device(V, ODD, u32(1), u64(0), u32(2), i(0), B, N, N), BAD),
            ("commit_device misaligned nodes" + tag, lambda V=V: L.lw_rpo_commit_columns_device(V, A, u32(1), u64(0), u32(2), i(0), ODD, N, N), BAD),
            # strides below the length
            ("hash_device row stride" + tag, lambda V=V: L.lw_rpo_hash_device(V, A, sz(2), sz(5), sz(4), B, N), BAD),
            ("commit_device column stride" + tag, lambda V=V: L.lw_rpo_commit_columns_device(V, A, u32(2), u64(3), u32(2), i(0), B, N, N), BAD),
            # sizes past what can be addressed
            ("commit 2^31 leaves" + tag, lambda V=V: L.lw_rpo_commit_columns(V, A, u32(1), u32(31), i(0), B, N), ALLOC),
            ("commit_device 2^31 leaves" + tag, lambda V=V: L.lw_rpo_commit_columns_device(V, A, u32(1), u64(0), u32(31), i(0), B, N, N), ALLOC),
            ("permute 2^36 + 1" + tag, lambda V=V: L.lw_rpo_permute(V, A, sz((1 << 36) + 1), B), ALLOC),
            ("hash row_len 2^31 + 1" + tag, lambda V=V: L.lw_rpo_hash(V, A, sz(1), sz((1 << 31) + 1), B), ALLOC),
        ]
    for bad in (-1, 2):
        V = i(bad)
        tag = " level %d" % bad
        cases += [
            ("permute" + tag, lambda V=V: L.lw_rpo_permute(V, A, sz(1), B), BAD),
            ("permute_device" + tag, lambda V=V: L.lw_rpo_permute_device(V, A, sz(1), B, N), BAD),
            ("permute n=0" + tag, lambda V=V: L.lw_rpo_permute(V, N, sz(0), N), BAD),
            ("hash" + tag, lambda V=V: L.lw_rpo_hash(V, A, sz(1), sz(2), B), BAD),
            ("hash_device" + tag, lambda V=V: L.lw_rpo_hash_device(V, A, sz(1), sz(2), sz(0), B, N), BAD),
            ("commit" + tag, lambda V=V: L.lw_rpo_commit_columns(V, A, u32(1), u32(2), i(0), B, N), BAD),
            ("commit_device" + tag, lambda V=V: L.lw_rpo_commit_columns_device(V, A, u32(1), u64(0), u32(2), i(0), B, N, N), BAD),
        ]
    got = {name: call() for name, call, _ in cases}
    assert got == {name: code for name, _, code in cases}
    assert len(got) == len(cases) and not buf.any()


# ---- 7. no device: an error, not a fallback
def test_host_forms_fail_loudly_without_a_device():
    import torch
    from lambda_elliptic_curves_amd import errors, rpo
    for level in (rpo.LEVEL_128, rpo.LEVEL_160):
        m = rpo.state_width(level)
        if not torch.cuda.is_available():
            with pytest.raises(errors.HipError):
                rpo.permute(level, np.zeros((1, m), np.uint64))
            with pytest.raises(errors.HipError):
                rpo.hash(level, np.arange(3, dtype=np.uint64))
            with pytest.raises(errors.HipError):
                rpo.hash_bytes(level, b"abc")
            with pytest.raises(errors.HipError):
                rpo.merge(level, np.zeros((1, rpo.digest_len(level)), np.uint64), np.ones((1, rpo.digest_len(level)), np.uint64))
            with pytest.raises(errors.HipError):
                rpo.commit_columns(level, np.zeros((2, 4), np.uint64))
        assert rpo.permute(level, np.zeros((0, m), np.uint64)).shape == (0, m)   # no work: no device needed
        assert rpo.hash(level, np.zeros((0, 5), np.uint64)).shape == (0, rpo.digest_len(level))
        with pytest.raises(errors.InputError):
            rpo.commit_columns(level, np.zeros((2, 3), np.uint64))
    with pytest.raises(ValueError):
        rpo.hash(2, np.zeros(3, np.uint64))
    assert (rpo.state_width(rpo.LEVEL_128), rpo.rate(rpo.LEVEL_128), rpo.digest_len(rpo.LEVEL_128)) == (12, 8, 4)
    assert (rpo.state_width(rpo.LEVEL_160), rpo.rate(rpo.LEVEL_160), rpo.digest_len(rpo.LEVEL_160)) == (16, 10, 5)


# ---- 8. hash_bytes: the host-side splitting is the reference's (utils.rs:8-21)
def test_bytes_to_field_elements():
    from lambda_elliptic_curves_amd import rpo
    f = lambda b: rpo.bytes_to_field_elements(b).tolist()
    assert f(b"") == []
    assert f(bytes([1, 2, 3])) == [1 | 2 << 8 | 3 << 16 | 1 << 24]
    assert f(bytes([1, 2, 3, 0])) == [1 | 2 << 8 | 3 << 16 | 1 << 32]
    assert f(bytes([1, 2, 3])) != f(bytes([1, 2, 3, 0]))                     # the padding pairs of the reference differ
    assert f(bytes(7)) == [0] and f(bytes(6)) == [1 << 48] and f(bytes(8)) == [0, 1 << 8]
    assert f(bytes(7)) != f(bytes(6)) and f(bytes(7)) != f(bytes(8))
    assert f(b"\xff" * 7) == [(1 << 56) - 1] and f(b"\xff" * 14) == [(1 << 56) - 1] * 2
    rng = np.random.default_rng(8)
    for length in range(0, 30):
        data = rng.bytes(length)
        assert f(data) == R.bytes_to_field_elements(data)
        assert len(f(data)) == (length + 6) // 7 and all(v < 1 << 56 for v in f(data))
    assert rpo.bytes_to_field_elements(bytearray(b"ab")).dtype == np.uint64
