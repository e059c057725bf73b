"""Monolith over Mersenne31 on the device (csrc/monolith.cuh, monolith.hip) against the reference's three recorded
vectors (tests/golden/monolith_mersenne31.json) and the restatement of tests/monolith_ref.py (integers for single states,
numpy for batches and trees; tests/test_monolith_cpu.py ties the two together).  Every comparison is bit for bit.

Launch boundaries of the tree (hash_tree.cuh): a workgroup is 256 work-items; the top kernel builds everything from a
level of 2^9 nodes (256 parents) down; every level above is one launch of the pair kernel.  log2n = 0 launches the leaf
kernel alone, 1 .. 9 add the top kernel, 10 adds one pair launch."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from lambda_elliptic_curves_amd import _lib as L
from lambda_elliptic_curves_amd import circle, fft, merkle, monolith
from tests import circle_ref
from tests import monolith_ref as M

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = M.P
ROUNDS = 5   # what the reference tests; the trees and hashes use it
TOP_LOG2 = 9


def dev(a):
    return torch.from_numpy(np.array(a, dtype=np.uint32, order="C").view(np.int32)).cuda()   # a copy: the shared references are read-only


def host(t):
    return t.cpu().numpy().view(np.uint32)


def empty(*shape):
    return torch.zeros(shape, dtype=torch.int32, device="cuda")


def rand_words(shape, seed):
    return np.random.default_rng(seed).integers(0, 1 << 32, shape, dtype=np.uint32)   # any u32: non-canonical words included


def assert_canonical(words):
    assert (np.asarray(words, np.uint32) < np.uint32(P)).all(), "a stored word is not below p"


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(ROOT, "tests", "golden", "monolith_mersenne31.json")) as f:
        return json.load(f)


# ---- 1. the reference's vectors through the ABI, host and device forms
def test_reference_vectors_through_the_abi(golden):
    v = golden["from_plonky3_width_16"]
    s = rand_words((257, 16), 1)
    lanes = [0, 63, 64, 256]
    s[lanes] = np.arange(16, dtype=np.uint32)
    got_h = monolith.permute(16, v["rounds"], s)
    got_d = host(monolith.permute_device(16, v["rounds"], dev(s), 257, empty(257, 16)))
    for lane in lanes:
        assert got_h[lane].tolist() == v["expected"] and got_d[lane].tolist() == v["expected"], lane
    assert np.array_equal(got_h, got_d) and np.array_equal(got_d, M.np_permute(16, v["rounds"], s))
    for name in ("from_plonky3_concrete_width_16", "from_plonky3_concrete_width_12"):
        w, r = golden[name]["width"], golden[name]["rounds"]
        s = rand_words((65, w), 2)
        s[[0, 64]] = np.arange(w, dtype=np.uint32)
        got = host(monolith.layer_device(w, r, monolith.LAYER_CONCRETE, dev(s), 65, empty(65, w)))
        assert got[0].tolist() == golden[name]["expected"] and got[64].tolist() == golden[name]["expected"], name
        assert np.array_equal(got, M.np_concrete(M.np_reduce(s), M.constants(w, r)[1]).astype(np.uint32))
    for w, r in ((16, 5), (12, 5), (8, 1), (24, 15)):   # the generated constants, with a device present too
        rc, mds = monolith.constants(w, r)
        assert rc.tolist() == M.constants(w, r)[0] and mds.tolist() == M.constants(w, r)[1]


# ---- 2. the seam: exact words in front of one layer
def test_seam_bars_every_byte_value_in_every_lane():
    words = M.bars_words()
    assert len(words) == 7 + 2 * (3 * 256 + 128) and max(words) == P
    n = -(-len(words) // 8)
    for w in (8, 16, 24):
        s = np.full((n, w), 0x12345678, np.uint32)
        s[:, :8] = np.array(words + [0] * (8 * n - len(words)), np.uint32).reshape(n, 8)
        exp = s.copy()
        exp[:, :8] = np.array([M.bar(int(x)) % P for x in s[:, :8].reshape(-1)], np.uint32).reshape(n, 8)   # p -> p, handed back as 0
        got = host(monolith.layer_device(w, ROUNDS, monolith.LAYER_BARS, dev(s), n, empty(n, w)))
        assert np.array_equal(got, exp), w
    assert M.bar(P) == P and M.bar(0) == 0


@pytest.mark.parametrize("width", [16, 24])
def test_seam_concrete_largest_accumulators(width):
    mds = M.constants(width, ROUNDS)[1]
    states = [[P] * width, [0xFFFFFFFF] * width, [P - 1] * width, [1 << 31] * width]
    states += rand_words((61, width), 3).tolist()
    s = np.array(states, np.uint32)
    got = host(monolith.layer_device(width, ROUNDS, monolith.LAYER_CONCRETE, dev(s), len(states), empty(len(states), width)))
    assert_canonical(got)
    assert got.tolist() == [M.concrete([M.reduce_word(x) for x in st], mds) for st in states]
    assert not got[0].any()                                             # all p is all zero
    assert got[1].tolist() == [sum(row) % P for row in mds]             # 2^32 - 1 is read as 1
    if width == 24:                                                     # the matrix follows the round count
        other = host(monolith.layer_device(width, 15, monolith.LAYER_CONCRETE, dev(s), len(states), empty(len(states), width)))
        assert other.tolist() == [M.concrete([M.reduce_word(x) for x in st], M.constants(width, 15)[1]) for st in states]
        assert not np.array_equal(other, got)


@pytest.mark.parametrize("width", M.WIDTHS)
def test_seam_bricks(width):
    states = [[P] * width, [P - 1] * width, [0xFFFFFFFF] * width] + rand_words((62, width), 4).tolist()
    s = np.array(states, np.uint32)
    t = dev(s)
    got = host(monolith.layer_device(width, ROUNDS, monolith.LAYER_BRICKS, t, len(states)))   # in place
    assert_canonical(got)
    assert got.tolist() == [M.bricks([M.reduce_word(x) for x in st]) for st in states]
    assert not got[0].any()


# ---- 3. the permutation: every width, few and many rounds, edge states and batches around the wave and the workgroup
@pytest.mark.parametrize("rounds", [1, 5, 15])
@pytest.mark.parametrize("width", M.WIDTHS)
def test_permute(width, rounds):
    edge = M.edge_states(width)
    assert len(edge) == 5 + width
    batches = [np.array(edge, np.uint32)] + [rand_words((n, width), 100 + n) for n in (1, 63, 64, 65, 1000)]
    s = np.concatenate(batches)
    exp = M.np_permute(width, rounds, s)
    assert exp[:len(edge)].tolist() == [M.permute(width, rounds, st) for st in edge]
    at = 0
    for b in batches:
        n = b.shape[0]
        want = exp[at:at + n]
        at += n
        t = dev(b)
        out = host(monolith.permute_device(width, rounds, t, n, torch.zeros_like(t)))
        assert_canonical(out)
        assert np.array_equal(out, want), n
        assert np.array_equal(host(t), b)                                      # out of place: the input is untouched
        assert np.array_equal(host(monolith.permute_device(width, rounds, t, n)), want), n   # out == states
    assert np.array_equal(monolith.permute(width, rounds, s), exp)


# ---- 4. hash: every chunk boundary, a row stride, 1 / 64 / 65 rows
@pytest.mark.parametrize("n_rows", [1, 64, 65])
def test_hash_every_row_length(n_rows):
    for row_len in list(range(0, 18)) + [24, 25]:
        rows = rand_words((n_rows, row_len), 40 + row_len)
        exp = M.np_hash(ROUNDS, rows)
        t_rows = dev(rows) if row_len else empty(4)
        out = host(monolith.hash_device(ROUNDS, t_rows, n_rows, row_len, empty(n_rows, 8) + 7))
        assert_canonical(out)
        assert np.array_equal(out, exp), row_len
        assert np.array_equal(monolith.hash(ROUNDS, rows), exp), row_len
        if row_len == 0:
            assert not out.any()
        stride = row_len + 3   # a row stride above the row length: the words between the rows are never read
        padded = np.full((n_rows, stride), 0xdeadbeef, np.uint32)
        padded[:, :row_len] = rows
        out = host(monolith.hash_device(ROUNDS, dev(padded), n_rows, row_len, empty(n_rows, 8), row_stride=stride))
        assert np.array_equal(out, exp), row_len
    assert exp[0].tolist() == M.hash(ROUNDS, [int(v) for v in rows[0]])
    assert monolith.hash(ROUNDS, rows[0]).tolist() == exp[0].tolist()   # a single sequence


def test_hash_and_compress_other_round_counts():
    rows = rand_words((65, 11), 60)
    left, right = rand_words((65, 8), 61), rand_words((65, 8), 62)
    for rounds in (1, 5, 15):
        assert np.array_equal(monolith.hash(rounds, rows), M.np_hash(rounds, rows))
        exp = M.np_compress(rounds, left, right)
        assert np.array_equal(monolith.compress(rounds, left, right), exp)
        out = host(monolith.compress_device(rounds, dev(left), dev(right), 65, empty(65, 8)))
        assert_canonical(out)
        assert np.array_equal(out, exp)
        assert exp[64].tolist() == M.compress(rounds, [int(v) for v in left[64]], [int(v) for v in right[64]])
    one = monolith.compress(ROUNDS, left[:1], right[:1])
    assert np.array_equal(one[0], monolith.permute(16, ROUNDS, np.concatenate([left[0], right[0]]))[0, :8])


# ---- 5. small trees, every node against the restatement
_TREES = {}
N_COLS = (1, 8, 9)   # one partial chunk, one full chunk, a full and a partial one


def ref_tree(n_cols, log2n, bit_reverse):
    """the restatement's tree over the columns of this (n_cols, log2n); both leaf orders are computed together, once"""
    if (n_cols, log2n, bit_reverse) not in _TREES:
        cols = rand_words((n_cols, 1 << log2n), 1000 + 16 * n_cols + log2n)
        cols.setflags(write=False)
        for br, nodes in zip((True, False), M.np_trees(ROUNDS, [M.committed_rows(cols, br) for br in (True, False)])):
            nodes.setflags(write=False)
            _TREES[(n_cols, log2n, br)] = (cols, nodes)
    return _TREES[(n_cols, log2n, bit_reverse)]


def device_tree(cols, bit_reverse, stride=0):
    n_cols, n = cols.shape
    if stride:
        padded = np.full((n_cols, stride), 0xdeadbeef, np.uint32)   # between the columns: never read
        padded[:, :n] = cols
        cols = padded
    t_nodes = empty(2 * n - 1, 8)
    root = monolith.commit_columns_device(ROUNDS, dev(cols), n_cols, n.bit_length() - 1, t_nodes, bit_reverse, col_stride=stride)
    nodes = host(t_nodes)
    assert np.array_equal(root, nodes[0])
    return nodes


@pytest.mark.parametrize("n_cols", N_COLS)
@pytest.mark.parametrize("log2n", range(0, TOP_LOG2 + 2))
def test_small_trees_every_node(log2n, n_cols):
    for bit_reverse in (True, False):
        cols, exp = ref_tree(n_cols, log2n, bit_reverse)
        nodes = device_tree(cols, bit_reverse)
        assert_canonical(nodes)
        assert np.array_equal(nodes, exp), bit_reverse
    if log2n > 1:
        assert not np.array_equal(ref_tree(n_cols, log2n, True)[1], ref_tree(n_cols, log2n, False)[1])


def test_tree_with_a_column_stride_and_the_host_form():
    for n_cols, log2n in ((8, 3), (9, TOP_LOG2 + 1)):
        cols, exp = ref_tree(n_cols, log2n, True)
        assert np.array_equal(device_tree(cols, True, stride=(1 << log2n) + 12), exp)
        root, nodes = monolith.commit_columns(ROUNDS, cols, True, return_nodes=True)   # the host form, all nodes returned
        assert np.array_equal(nodes, exp) and np.array_equal(root, exp[0])
        assert np.array_equal(monolith.commit_columns(ROUNDS, cols, True), exp[0])
    cols, exp = ref_tree(1, 2, True)
    leaves = [M.hash(ROUNDS, [int(cols[0, j])]) for j in (0, 2, 1, 3)]   # one tree tied to the integer form by hand
    l01, l23 = M.compress(ROUNDS, leaves[0], leaves[1]), M.compress(ROUNDS, leaves[2], leaves[3])
    assert exp.tolist() == [M.compress(ROUNDS, l01, l23), l01, l23] + leaves


FIRST_CALL = """
import sys, numpy as np, torch
from lambda_elliptic_curves_amd import monolith
cols = np.frombuffer(bytes.fromhex(sys.argv[1]), np.int32).reshape(2, 8)
t_nodes = torch.zeros((15, 8), dtype=torch.int32, device="cuda")
monolith.commit_columns_device(5, torch.from_numpy(cols.copy()).cuda(), 2, 3, t_nodes)
print(t_nodes.cpu().numpy().tobytes().hex())
"""


def test_the_first_call_of_a_process_may_be_a_device_tree():
    """The constants are uploaded inside the tree call (MonolithHash::ready), under the call's one hold of the lane: a
    process whose first library call is commit_columns_device gets all 15 nodes right.  A tree built against a table that
    is not there hashes against zeros."""
    cols, exp = ref_tree(2, 3, True)
    out = subprocess.run([sys.executable] + (["-s"] if sys.flags.no_user_site else []) + ["-c", FIRST_CALL, cols.tobytes().hex()],
                         cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    assert np.array_equal(np.frombuffer(bytes.fromhex(out.stdout.split()[-1]), np.uint32).reshape(15, 8), exp)


# ---- 6. circle LDE -> commit on the resident output -> authentication paths read from the resident tree
def test_lde_then_commit_resident_and_open():
    n_cols, log2c, log2n = 3, 8, 10
    n = 1 << log2n
    evals = rand_words((n_cols, 1 << log2c), 91)
    t_lde = empty(n_cols, n)
    circle.lde_device(dev(evals), log2c, t_lde, log2n, batch=n_cols)
    t_nodes = empty(2 * n - 1, 8)
    root = monolith.commit_columns_device(ROUNDS, t_lde, n_cols, log2n, t_nodes, True)
    lde = host(t_lde)
    assert np.array_equal(lde, circle_ref.np_lde(evals, log2n))
    exp = M.np_tree(ROUNDS, lde, True)
    assert np.array_equal(root, exp[0])
    nodes_h = host(t_nodes)
    assert np.array_equal(nodes_h, exp)
    # the paths through the existing call: 32-byte nodes, root first, no columns
    positions = [0, n - 1] + [int(x) for x in np.random.default_rng(78).integers(0, n, 6)]
    tree = merkle.Tree(fft.Stark252PrimeField, t_nodes, log2n)
    _, paths = merkle.open_trees_device([tree], np.array(positions, np.uint64))
    assert paths[0].shape == (len(positions), log2n, 32)
    for q, pos in enumerate(positions):
        cur = M.hash(ROUNDS, [int(v) for v in lde[:, M.bitrev(pos, log2n)]])
        assert cur == nodes_h[n - 1 + pos].tolist()
        i = pos
        for sib in paths[0][q].view(np.uint32).reshape(log2n, 8).tolist():
            cur = M.compress(ROUNDS, cur, sib) if i % 2 == 0 else M.compress(ROUNDS, sib, cur)
            i >>= 1
        assert cur == root.tolist(), pos


# ---- 7. misaligned device pointers, bad widths and round counts are rejected before any launch
def test_misaligned_device_pointers_widths_and_rounds():
    lib = L.lib()
    t = torch.zeros(4096, dtype=torch.int32, device="cuda")
    ok, off = t.data_ptr(), t.data_ptr() + 4
    assert ok % 16 == 0
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    BAD = L.ERR_BAD_ARG
    for a, b in ((off, ok + 4096), (ok, off + 4096), (ok + 8, ok + 4096)):
        assert lib.lw_monolith_permute_device(16, 5, a, 1, b, s) == BAD
        assert lib.lw_monolith_layer_device(16, 5, 1, a, 1, b, s) == BAD
        assert lib.lw_monolith_hash_device(5, a, 1, 2, 0, b, s) == BAD
        assert lib.lw_monolith_compress_device(5, a, ok + 8192, 1, b, s) == BAD
        assert lib.lw_monolith_commit_columns_device(5, a, 1, 0, 2, 0, b, None, s) == BAD
    for width in (0, 4, 10, 28):
        assert lib.lw_monolith_permute_device(width, 5, ok, 1, ok + 4096, s) == BAD
        assert lib.lw_monolith_layer_device(width, 5, 0, ok, 1, ok + 4096, s) == BAD
    for rounds in (0, 16):
        assert lib.lw_monolith_permute_device(16, rounds, ok, 1, ok + 4096, s) == BAD
        assert lib.lw_monolith_hash_device(rounds, ok, 1, 2, 0, ok + 4096, s) == BAD
        assert lib.lw_monolith_compress_device(rounds, ok, ok + 8192, 1, ok + 4096, s) == BAD
        assert lib.lw_monolith_commit_columns_device(rounds, ok, 1, 0, 2, 0, ok + 4096, None, s) == BAD
    assert lib.lw_monolith_layer_device(16, 5, 3, ok, 1, ok + 4096, s) == BAD
    torch.cuda.synchronize()
    assert not t.any()
