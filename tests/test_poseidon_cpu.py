"""Starknet Poseidon without a device: the big-integer model (tests/poseidon_ref.py) against the reference's fixed vectors,
the generated round keys against their definition, and the argument checks of the C entry points."""
import ctypes as C
import hashlib
import json
import os
import re

import numpy as np

from tests import poseidon_ref as R
from tools import gen_poseidon_consts as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def golden():
    with open(os.path.join(ROOT, "tests", "golden", "poseidon_starknet.json")) as f:
        return json.load(f)


def h(s):
    return int(s, 16)


def test_model_reproduces_the_reference_vectors():
    g = golden()
    assert len(g["permutation"]) == 1 and len(g["hash"]) == 1 and len(g["hash_single"]) == 1 and len(g["hash_many"]) == 5
    for c in g["permutation"]:
        assert R.permute([h(x) for x in c["state"]]) == [h(x) for x in c["expected"]], c["cite"]
    for c in g["hash"]:
        assert R.hash2(h(c["x"]), h(c["y"])) == h(c["expected"]), c["cite"]
    for c in g["hash_single"]:
        assert R.hash_single(h(c["x"])) == h(c["expected"]), c["cite"]
    for c in g["hash_many"]:
        assert R.hash_many([h(x) for x in c["inputs"]]) == h(c["expected"]), c["cite"]


def test_poseidon_consts_inc_matches_generator():
    with open(G.output_path()) as f:
        committed = f.read()
    assert G.render() == committed, "poseidon_consts.inc is stale: run python3 tools/gen_poseidon_consts.py"


def test_committed_constants_follow_the_sha256_rule():
    # parsed from the committed file, taken out of Montgomery form, compared with the rule spelled out here once more
    with open(G.output_path()) as f:
        rows = re.findall(r"^\{([^}]*)\}", f.read(), re.M)
    assert len(rows) == 91 * 3
    p = 2**251 + 17 * 2**192 + 1
    r_inv = pow(2**256, -1, p)
    for idx, row in enumerate(rows):
        limbs = [int(w.strip().rstrip("u"), 16) for w in row.split(",")]
        assert len(limbs) == 8 and all(0 <= w < 2**32 for w in limbs)
        m = sum(w << (32 * k) for k, w in enumerate(limbs))   # least significant limb first
        assert m < p, idx
        assert m * r_inv % p == int(hashlib.sha256(("Hades" + str(idx)).encode()).hexdigest(), 16) % p, idx
        assert m * r_inv % p == R.KEYS[idx // 3][idx % 3]


def test_model_layout_round_trip():
    vals = [0, 1, 2, R.P - 1, 0x123456]
    e = R.to_elems(vals)
    assert e.shape == (5, 4) and R.from_elems(e) == vals
    assert R.raw_ints(e[1:2]) == [2**256 % R.P]   # one in Montgomery form, most significant limb first


def test_argument_codes_need_no_device():
    from lambda_elliptic_curves_amd import _lib
    L = C.CDLL(_lib.LIB_PATH)   # a handle of its own: plain ctypes arguments, no argtypes
    buf = np.zeros(4096, np.uint8)
    assert buf.ctypes.data % 16 == 0
    P, Q, N = C.c_void_p(buf.ctypes.data), C.c_void_p(buf.ctypes.data + 2048), C.c_void_p(None)
    i, u32, u64, sz = C.c_int, C.c_uint32, C.c_uint64, C.c_size_t
    SINGLE, MANY = i(_lib.POSEIDON_LEAF_SINGLE), i(_lib.POSEIDON_LEAF_MANY)
    BAD, ALLOC, OK = _lib.ERR_BAD_ARG, _lib.ERR_ALLOC, _lib.OK
    cases = [
        # n = 0 / n_rows = 0: nothing to do, nothing touched (null buffers included)
        ("permute n=0", lambda: L.lw_poseidon_permute(N, sz(0), N), OK),
        ("permute_device n=0", lambda: L.lw_poseidon_permute_device(N, sz(0), N, N), OK),
        ("hash n=0", lambda: L.lw_poseidon_hash(N, N, sz(0), N), OK),
        ("hash_device n=0", lambda: L.lw_poseidon_hash_device(N, N, sz(0), N, N), OK),
        ("hash_single n=0", lambda: L.lw_poseidon_hash_single(N, sz(0), N), OK),
        ("hash_single_device n=0", lambda: L.lw_poseidon_hash_single_device(N, sz(0), N, N), OK),
        ("hash_many n_rows=0", lambda: L.lw_poseidon_hash_many(N, sz(0), sz(3), N), OK),
        ("hash_many_device n_rows=0", lambda: L.lw_poseidon_hash_many_device(N, sz(0), sz(3), N, N), OK),
        # null pointers
        ("permute null in", lambda: L.lw_poseidon_permute(N, sz(1), P), BAD),
        ("permute null out", lambda: L.lw_poseidon_permute(P, sz(1), N), BAD),
        ("permute_device null", lambda: L.lw_poseidon_permute_device(N, sz(1), P, N), BAD),
        ("hash null y", lambda: L.lw_poseidon_hash(P, N, sz(1), Q), BAD),
        ("hash_device null out", lambda: L.lw_poseidon_hash_device(P, P, sz(1), N, N), BAD),
        ("hash_single null", lambda: L.lw_poseidon_hash_single(N, sz(1), P), BAD),
        ("hash_single_device null", lambda: L.lw_poseidon_hash_single_device(P, sz(1), N, N), BAD),
        ("hash_many null rows", lambda: L.lw_poseidon_hash_many(N, sz(1), sz(2), P), BAD),
        ("hash_many null out", lambda: L.lw_poseidon_hash_many(P, sz(1), sz(0), N), BAD),
        ("hash_many_device null rows", lambda: L.lw_poseidon_hash_many_device(N, sz(1), sz(2), P, N), BAD),
        ("commit null columns", lambda: L.lw_poseidon_commit_columns(N, u32(1), u32(2), i(0), MANY, P, N), BAD),
        ("commit null root", lambda: L.lw_poseidon_commit_columns(P, u32(1), u32(2), i(0), MANY, N, N), BAD),
        ("commit_device null nodes", lambda: L.lw_poseidon_commit_columns_device(P, u32(1), u64(0), u32(2), i(0), MANY, N, N, N), BAD),
        ("commit no columns", lambda: L.lw_poseidon_commit_columns(P, u32(0), u32(2), i(0), MANY, P, N), BAD),
        # leaf modes
        ("commit single, 2 columns", lambda: L.lw_poseidon_commit_columns(P, u32(2), u32(2), i(0), SINGLE, Q, N), BAD),
        ("commit_device single, 2 columns", lambda: L.lw_poseidon_commit_columns_device(P, u32(2), u64(0), u32(2), i(0), SINGLE, Q, N, N), BAD),
        ("commit bad leaf mode", lambda: L.lw_poseidon_commit_columns(P, u32(1), u32(2), i(0), i(2), Q, N), BAD),
        ("commit_device bad leaf mode", lambda: L.lw_poseidon_commit_columns_device(P, u32(1), u64(0), u32(2), i(0), i(-1), Q, N, N), BAD),
        # columns that would overlap
        ("commit_device column stride", lambda: L.lw_poseidon_commit_columns_device(P, u32(2), u64(3), u32(2), i(0), MANY, Q, N, N), BAD),
        # sizes past what can be addressed
        ("commit 2^32 leaves", lambda: L.lw_poseidon_commit_columns(P, u32(1), u32(32), i(0), MANY, Q, N), ALLOC),
        ("commit_device 2^32 leaves", lambda: L.lw_poseidon_commit_columns_device(P, u32(1), u64(0), u32(32), i(0), SINGLE, Q, N, N), ALLOC),
        ("permute 2^36 + 1", lambda: L.lw_poseidon_permute(P, sz((1 << 36) + 1), Q), ALLOC),
        ("hash_many row_len 2^31 + 1", lambda: L.lw_poseidon_hash_many(P, sz(1), sz((1 << 31) + 1), Q), ALLOC),
    ]
    got = {name: call() for name, call, _ in cases}
    assert got == {name: code for name, _, code in cases}
    assert not buf.any()


def test_host_forms_fail_loudly_without_a_device():
    import pytest
    import torch
    from lambda_elliptic_curves_amd import errors, poseidon
    one = R.to_elems([1])
    if not torch.cuda.is_available():   # no CPU fallback: with work to do and no device, the host forms raise
        with pytest.raises(errors.HipError):
            poseidon.hash(one, one)
        with pytest.raises(errors.HipError):
            poseidon.commit_columns(one.reshape(1, 1, 4), poseidon.LEAF_SINGLE)
    assert poseidon.permute(np.zeros((0, 3, 4), np.uint64)).shape == (0, 3, 4)   # no work: no device needed
