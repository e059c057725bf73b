"""Device-free checks of the STARK round 4 tail (stark_query.hip): the Python restatement against the reference's grinding
vectors and recorded authentication path, and every argument check of the new entry points, which must answer before any
device is touched."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from oracle import oracle as O
from tests import stark_query_ref as R
from tests import util

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def grinding():
    with open(os.path.join(ROOT, "tests", "golden", "stark_grinding.json")) as f:
        g = json.load(f)
    g["seeds"] = {k: bytes(v) for k, v in g["seeds"].items()}
    return g


def test_restatement_reproduces_the_reference_vectors(grinding):
    for v in grinding["valid"]:
        assert R.is_valid_nonce(grinding["seeds"][v["seed"]], int(v["nonce"], 16), v["grinding_factor"]), v
    for v in grinding["invalid"]:
        assert not R.is_valid_nonce(grinding["seeds"][v["seed"]], int(v["nonce"], 16), v["grinding_factor"]), v


def test_restatement_smallest_nonces_up_to_factor_12(grinding):
    for name, row in grinding["smallest"].items():
        for g, nonce in row.items():
            nonce = int(nonce, 16)
            assert R.is_valid_nonce(grinding["seeds"][name], nonce, int(g)), (name, g)
            if int(g) <= 12:
                assert R.smallest_nonce(grinding["seeds"][name], int(g)) == nonce, (name, g)


def test_restatement_reproduces_the_full_width_nonces(grinding):
    """the pointwise validities and the searches above 2^32 that tests/test_gpu_stark_query.py asks of the device"""
    nonces = [int(x, 16) for x in grinding["pointwise"]["nonces"]]
    assert nonces == R.pointwise_nonces() and max(nonces) == 2**64 - 2
    assert {1 << k for k in range(64)} | {0xff << (8 * j) for j in range(8)} | {2**32 - 1, 2**32, 2**32 + 1} <= set(nonces)
    assert sum(1 for x in nonces if x >= 2**32) == 40       # bswap64 of these has a low half that is not zero
    for name, rows in grinding["pointwise"]["valid"].items():
        assert sorted(rows) == ["1", "2", "3", "4"]
        for g, row in rows.items():
            inner = R.inner_hash(grinding["seeds"][name], int(g))
            assert row == "".join("01"[R.is_valid_nonce(grinding["seeds"][name], x, int(g), inner)] for x in nonces), (name, g)
            assert "0" in row and "1" in row
    assert len(grinding["searches"]) == 13
    for s in grinding["searches"]:
        first, last = int(s["first"], 16), int(s["last"], 16)
        assert 2**32 <= first <= last <= 2**64 - 2
        want = None if s["nonce"] is None else int(s["nonce"], 16)
        assert R.smallest_nonce(grinding["seeds"][s["seed"]], s["grinding_factor"], first, last) == want, s
    offsets = {(int(s["first"], 16), s["seed"]): int(s["nonce"], 16) - int(s["first"], 16) for s in grinding["searches"]
               if s["grinding_factor"] == 8 and int(s["last"], 16) == int(s["first"], 16) + 5000}
    assert offsets == {(2**32, "A"): 141, (2**32, "B"): 254, (2**40 + 12345, "A"): 417, (2**40 + 12345, "B"): 212,
                       (2**63, "A"): 194, (2**63, "B"): 546, (2**64 - 2**20, "A"): 200, (2**64 - 2**20, "B"): 513}
    # 2^64 - 1 would be valid for seed B at factor 1; the reference never tries it, and neither does the library
    assert R.is_valid_nonce(grinding["seeds"]["B"], 2**64 - 1, 1) and R.is_valid_nonce(grinding["seeds"]["B"], 2**64 - 2, 1)


def test_the_documents_say_that_the_largest_u64_is_no_candidate():
    from lambda_elliptic_curves_amd import stark
    header = " ".join(open(os.path.join(ROOT, "include", "lw_hip.h")).read().replace("*", " ").split())
    assert "2^64 - 1 is never a candidate" in header and "means 2^64 - 2" in header
    doc = " ".join(stark.grinding_nonce.__doc__.split())
    assert "2^64 - 1 is never a candidate" in doc and "last = 2^64 - 1 means 2^64 - 2" in doc


# proof.deep_poly_openings[0].main_trace_polys.evaluations of the same proof (provers/stark/src/prover.rs:1438-1453)
STONE_CASE_1_EVALUATIONS = [0x4de0d56f9cf97dff326c26592fbd4ae9ee756080b12c51cfe4864e9b8734f43,
                            0x1bc1aadf39f2faee64d84cb25f7a95d3dceac1016258a39fc90c9d370e69e8e]


def stone_case_1_opening(kats):
    """The leaf position of the recorded opening: the even position (open_trace_polys opens 2 iota) whose row holds the
    recorded evaluations.  -> (pos, path)"""
    case = kats["stone_compat_trace_commitments"]["cases"][0]
    oid = O.F_STARK252
    n, blow = case["trace_length"], case["blowup_factor"]
    off = O.elems_to_mont(oid, [case["coset_offset"]])[0]
    cols = np.stack([O.evaluate_fft(oid, O.interpolate_fft(oid, O.elems_to_mont(oid, col)), blow, n, off)
                     for col in util.stone_compat_trace_columns(case["initial"], n)])
    log2_rows = (n * blow).bit_length() - 1
    want = O.elems_to_mont(oid, STONE_CASE_1_EVALUATIONS)
    rows = [j for j in range(n * blow) if np.array_equal(cols[:, R.bitrev(j, log2_rows)], want)]
    assert len(rows) == 1 and rows[0] % 2 == 0
    return case, cols, rows[0]


def test_merkle_path_reproduces_the_stone_compat_auth_path(kats):
    case, cols, pos = stone_case_1_opening(kats)
    nodes = O.merkle_commit_columns(cols, bit_reverse=True)
    path = R.merkle_path(nodes, pos)
    assert [bytes(x).hex() for x in path[1:4]] == case["auth_path_nodes"]
    assert R.fold_path(nodes[nodes.shape[0] // 2 + pos], pos, path).hex() == case["root"]


def test_merkle_path_shapes():
    rng = np.random.default_rng(5)
    assert R.merkle_path(rng.integers(0, 256, (1, 32), dtype=np.uint8), 0).shape == (0, 32)
    nodes = rng.integers(0, 256, (15, 32), dtype=np.uint8)
    assert np.array_equal(R.merkle_path(nodes, 0), nodes[[8, 4, 2]])
    assert np.array_equal(R.merkle_path(nodes, 7), nodes[[13, 5, 1]])


def test_argument_checks_do_not_need_a_device():
    from lambda_elliptic_curves_amd import _lib
    L = C.CDLL(_lib.LIB_PATH)   # a handle of its own: plain ctypes arguments
    u32, u64, N = C.c_uint32, C.c_uint64, C.c_void_p(None)
    seed = (C.c_uint8 * 32)()
    nonce, found = C.c_uint64(77), C.c_int(5)
    host = lambda g, first, last, s=seed, o=C.byref(nonce), f=C.byref(found): L.lw_stark_grinding_nonce(s, u32(g), u64(first), u64(last), o, f)
    dev = lambda g, first, last, s=seed, o=C.byref(nonce), f=C.byref(found): L.lw_stark_grinding_nonce_device(s, u32(g), u64(first), u64(last), o, f, N)
    cases = []
    for name, fn in (("grinding", host), ("grinding_device", dev)):
        cases += [
            (name + " factor 0", lambda fn=fn: fn(0, 0, 10), _lib.ERR_BAD_ARG),
            (name + " factor 64", lambda fn=fn: fn(64, 0, 10), _lib.ERR_BAD_ARG),
            (name + " null seed", lambda fn=fn: fn(8, 0, 10, s=N), _lib.ERR_BAD_ARG),
            (name + " null nonce", lambda fn=fn: fn(8, 0, 10, o=N), _lib.ERR_BAD_ARG),
            (name + " null found", lambda fn=fn: fn(8, 0, 10, f=N), _lib.ERR_BAD_ARG),
            (name + " first > last", lambda fn=fn: fn(8, 11, 10), _lib.ERR_BAD_ARG),
        ]
    buf = np.zeros(4096, np.uint8)
    P = buf.ctypes.data + (-buf.ctypes.data % 16)
    out_v, out_p = C.c_void_p(P + 1024), C.c_void_p(P + 2048)

    def open_(field=0, cols=P, n_cols=1, stride=0, log2_rows=3, rpl=1, nodes=P, pos=(0, 1), n_trees=1, q=2):
        tree = _lib.StarkTree(field, cols, n_cols, stride, log2_rows, rpl, 1, nodes)
        positions = (C.c_uint64 * max(len(pos), 1))(*pos)
        return L.lw_stark_open_trees_device(C.byref(tree), u32(n_trees), positions, u32(q), out_v, out_p, N)

    cases += [
        ("open position = leaves", lambda: open_(pos=(0, 8)), _lib.ERR_BAD_ARG),
        ("open position = leaves, two rows per leaf", lambda: open_(rpl=2, pos=(4, 0)), _lib.ERR_BAD_ARG),
        ("open rows_per_leaf 0", lambda: open_(rpl=0), _lib.ERR_BAD_ARG),
        ("open rows_per_leaf 3", lambda: open_(rpl=3), _lib.ERR_BAD_ARG),
        ("open one row, two per leaf", lambda: open_(log2_rows=0, rpl=2, pos=(0, 0)), _lib.ERR_BAD_ARG),
        ("open babybear", lambda: open_(field=2), _lib.ERR_BAD_ARG),
        ("open field 9", lambda: open_(field=9), _lib.ERR_BAD_ARG),
        ("open null nodes", lambda: open_(nodes=None), _lib.ERR_BAD_ARG),
        ("open q = 0", lambda: open_(q=0), _lib.OK),
        ("open n_trees = 0", lambda: open_(n_trees=0), _lib.OK),
        ("open q = 0, bad tree", lambda: open_(q=0, rpl=7, nodes=None), _lib.OK),
    ]
    got = {name: call() for name, call, _ in cases}
    assert got == {name: code for name, _, code in cases}
    assert (nonce.value, found.value) == (77, 5)          # nothing written by a rejected call
    assert not buf.any()


def test_python_wrappers_need_no_device_for_empty_calls():
    from lambda_elliptic_curves_amd import fft, merkle, stark
    assert merkle.open_trees_device([], np.zeros((0, 3), np.uint64)) == ([], [])
    assert stark.fri_query_phase_device(fft.Stark252PrimeField, [], [1, 2]) == []
    assert stark.open_deep_composition_poly_device(fft.Stark252PrimeField, None, None, []) == []
    assert stark.grinding_window(20) == 1 << 21 and stark.grinding_window(1) == 1 << 20 and stark.grinding_window(63) == 1 << 28
