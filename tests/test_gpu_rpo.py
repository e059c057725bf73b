"""Rescue Prime Optimized on the device (csrc/rpo.cuh, rpo.hip) against the reference's 38 fixed digests
(tests/golden/rpo_goldilocks.json) and the restatement of tests/rpo_ref.py (integers for single rows, numpy for batches
and trees).  Every comparison is bit for bit.

Launch boundaries of the tree (rpo_commit_device): a workgroup is 256 work-items; the top kernel builds everything from
a level of 2^9 nodes (256 parents) down; every level above is one launch of the pair kernel.  log2n = 0 launches the leaf
kernel alone, 1 .. 9 add the top kernel, 10 adds one pair launch, 11 is the smallest tree with two."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

from lambda_elliptic_curves_amd import _lib as L
from lambda_elliptic_curves_amd import fft, goldilocks, merkle, rpo
from tests import goldilocks_ref as G
from tests import rpo_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = R.P
LEVELS = [rpo.LEVEL_128, rpo.LEVEL_160]
BATCH, LANES = 257, (0, 63, 64, 256)   # a second workgroup, a partial last wave, not a multiple of 64
TOP_LOG2 = 9


def dev(a):
    return torch.from_numpy(np.array(a, dtype=np.uint64, order="C").view(np.int64)).cuda()   # a copy: the shared references are read-only


def host(t):
    return t.cpu().numpy().view(np.uint64)


def empty(*shape):
    return torch.zeros(shape, dtype=torch.int64, device="cuda")


def rand_words(shape, seed):
    return np.random.default_rng(seed).integers(0, 1 << 64, shape, dtype=np.uint64)   # any u64: non-canonical words included


def assert_canonical(words):
    assert (np.asarray(words, np.uint64) < np.uint64(P)).all(), "a stored word is not below p"


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(ROOT, "tests", "golden", "rpo_goldilocks.json")) as f:
        g = json.load(f)
    return {rpo.LEVEL_128: [[int(x) for x in row] for row in g["EXPECTED_128"]],
            rpo.LEVEL_160: [[int(x) for x in row] for row in g["EXPECTED_160"]]}


_TREES = {}


def tree_n_cols(level):
    return (1, rpo.rate(level), rpo.rate(level) + 1)   # one partial block, one full block, a full and a partial one


def ref_tree(level, n_cols, log2n, bit_reverse):
    """the restatement's tree over the columns of this (level, n_cols, log2n); both leaf orders are computed together,
    once"""
    if (level, n_cols, log2n, bit_reverse) not in _TREES:
        cols = rand_words((n_cols, 1 << log2n), 1000 + 64 * level + 16 * n_cols + log2n)
        cols.setflags(write=False)
        for br, nodes in zip((True, False), R.np_trees(level, [R.committed_rows(cols, br) for br in (True, False)])):
            nodes.setflags(write=False)
            _TREES[(level, n_cols, log2n, br)] = (cols, nodes)
    return _TREES[(level, n_cols, log2n, bit_reverse)]


# ---- 1. the reference's fixed digests through the host and the _device forms, at the lanes of LANES
@pytest.mark.parametrize("level", LEVELS)
def test_fixed_digests_through_the_abi(golden, level):
    d = rpo.digest_len(level)
    for i, exp in enumerate(golden[level]):
        length = i + 1
        rows = rand_words((BATCH, length), 10 + i)
        rows[list(LANES)] = np.arange(length, dtype=np.uint64)
        got_h = rpo.hash(level, rows)
        got_d = host(rpo.hash_device(level, dev(rows), BATCH, length, empty(BATCH, d)))
        for lane in LANES:
            assert got_h[lane].tolist() == exp and got_d[lane].tolist() == exp, (level, i, lane)
        assert np.array_equal(got_h, got_d)
        if i in (0, 7, 18):   # the random rows elsewhere, against the restatement
            assert np.array_equal(got_d, R.np_hash(level, rows))
        assert_canonical(got_d)
    assert rpo.hash(level, np.arange(3, dtype=np.uint64)).tolist() == golden[level][2]   # a single sequence


@pytest.mark.parametrize("level", LEVELS)
def test_hash_bytes_and_merge(level):
    for data in (b"", b"\x01\x02\x03", b"\x01\x02\x03\x00", bytes(7), bytes(range(40))):
        assert rpo.hash_bytes(level, data).tolist() == R.hash_bytes(level, data), data
    assert rpo.hash_bytes(level, b"\x01\x02\x03").tolist() != rpo.hash_bytes(level, b"\x01\x02\x03\x00").tolist()
    d = rpo.digest_len(level)
    left, right = rand_words((65, d), 31), rand_words((65, d), 32)
    exp = R.np_merge(level, left, right)
    assert np.array_equal(rpo.merge(level, left, right), exp)
    pairs = np.concatenate([left, right], axis=1)
    assert np.array_equal(host(rpo.merge_device(level, dev(pairs), 65, empty(65, d))), exp)
    assert exp[0].tolist() == R.hash(level, [int(v) for v in left[0]] + [int(v) for v in right[0]])


# ---- 2. the permutation on edge states, out of place and in place
@pytest.mark.parametrize("level", LEVELS)
def test_permute_edge_states(level):
    m = rpo.state_width(level)
    states = R.edge_states(level)
    assert len(states) == 4 + 2 * len(G.EDGE)
    s = np.array(states, np.uint64)
    exp = [R.permute(level, st) for st in states]
    assert np.array_equal(R.np_permute(level, s), np.array(exp, np.uint64))
    t = dev(s)
    out = host(rpo.permute_device(level, t, len(states), torch.zeros_like(t)))
    assert_canonical(out)
    assert out.tolist() == exp
    assert np.array_equal(host(t), s)                                   # out of place: the input is untouched
    inplace = host(rpo.permute_device(level, t, len(states)))           # out == states
    assert np.array_equal(inplace, out)
    assert np.array_equal(rpo.permute(level, s), out)
    assert s.shape == (len(states), m)


@pytest.mark.parametrize("level", LEVELS)
def test_permute_random_batch(level):
    m = rpo.state_width(level)
    s = rand_words((BATCH, m), 5)
    exp = R.np_permute(level, s)
    out = host(rpo.permute_device(level, dev(s), BATCH))
    assert_canonical(out)
    assert np.array_equal(out, exp)
    assert np.array_equal(rpo.permute(level, s), exp)


# ---- 3. hash: every padding branch, a row stride, 1 / 64 / 65 rows
@pytest.mark.parametrize("level", LEVELS)
@pytest.mark.parametrize("n_rows", [1, 64, 65])
def test_hash_every_row_length(level, n_rows):
    d, rt = rpo.digest_len(level), rpo.rate(level)
    for row_len in range(0, 2 * rt + 2):
        rows = rand_words((n_rows, row_len), 40 + row_len)
        exp = R.np_hash(level, rows)
        t_rows = dev(rows) if row_len else empty(2)
        out = host(rpo.hash_device(level, t_rows, n_rows, row_len, empty(n_rows, d) + 7))
        assert_canonical(out)
        assert np.array_equal(out, exp), row_len
        assert np.array_equal(rpo.hash(level, rows), exp), row_len
        if row_len == 0:
            assert not out.any()
        stride = row_len + 3   # a row stride above the row length: the words between the rows are never read
        padded = np.full((n_rows, stride), 0xdeadbeefdeadbeef, np.uint64)
        padded[:, :row_len] = rows
        out = host(rpo.hash_device(level, dev(padded), n_rows, row_len, empty(n_rows, d), row_stride=stride))
        assert np.array_equal(out, exp), row_len
    assert R.np_hash(level, rows[:1])[0].tolist() == R.hash(level, [int(v) for v in rows[0]])


# ---- 4. small trees, every node against the restatement
def device_tree(level, cols, bit_reverse, stride=0):
    n_cols, n = cols.shape
    if stride:
        padded = np.full((n_cols, stride), 0xdeadbeefdeadbeef, np.uint64)   # between the columns: never read
        padded[:, :n] = cols
        cols = padded
    t_nodes = empty(2 * n - 1, rpo.digest_len(level))
    root = rpo.commit_columns_device(level, dev(cols), n_cols, n.bit_length() - 1, t_nodes, bit_reverse, col_stride=stride)
    nodes = host(t_nodes)
    assert np.array_equal(root, nodes[0])
    return nodes


@pytest.mark.parametrize("which", [0, 1, 2])   # n_cols = 1, rate, rate + 1
@pytest.mark.parametrize("log2n", range(0, TOP_LOG2 + 2))
@pytest.mark.parametrize("level", LEVELS)
def test_small_trees_every_node(level, log2n, which):
    n_cols = tree_n_cols(level)[which]
    for bit_reverse in (True, False):
        cols, exp = ref_tree(level, n_cols, log2n, bit_reverse)
        nodes = device_tree(level, cols, bit_reverse)
        assert_canonical(nodes)
        assert np.array_equal(nodes, exp), bit_reverse
    if log2n > 1:
        assert not np.array_equal(ref_tree(level, n_cols, log2n, True)[1], ref_tree(level, n_cols, log2n, False)[1])


@pytest.mark.parametrize("level", LEVELS)
def test_tree_with_a_column_stride(level):
    for n_cols, log2n in ((rpo.rate(level), 3), (rpo.rate(level) + 1, TOP_LOG2 + 1)):
        cols, exp = ref_tree(level, n_cols, log2n, True)
        assert np.array_equal(device_tree(level, cols, True, stride=(1 << log2n) + 6), exp)
    cols, exp = ref_tree(level, 1, 2, True)
    leaves = [R.hash(level, [int(cols[0, j])]) for j in (0, 2, 1, 3)]   # one tree tied to the integer form by hand
    l01, l23 = R.hash(level, leaves[0] + leaves[1]), R.hash(level, leaves[2] + leaves[3])
    assert exp.tolist() == [R.hash(level, l01 + l23), l01, l23] + leaves


# ---- 5. the smallest tree with more than one wide level launch: 8 x 2^11
@pytest.mark.parametrize("level", LEVELS)
def test_larger_tree_levels_host_form_and_openings(level):
    n_cols, log2n = 8, TOP_LOG2 + 2
    n, d = 1 << log2n, rpo.digest_len(level)
    cols = rand_words((n_cols, n), 77)
    t_cols, t_nodes = dev(cols), empty(2 * n - 1, d)
    root = rpo.commit_columns_device(level, t_cols, n_cols, log2n, t_nodes, True)
    # (a) every level from the level below with the flat device calls (tied to the restatement by the tests above)
    perm = np.array([G.bitrev(j, log2n) for j in range(n)])
    leaves = rpo.hash_device(level, dev(cols.T[perm]), n, n_cols, empty(n, d))
    assert torch.equal(t_nodes[n - 1:], leaves)
    for m in range(log2n, 0, -1):
        children = t_nodes[(1 << m) - 1:(1 << (m + 1)) - 1].clone()   # a buffer of its own: 40-byte digests leave the slice misaligned
        parents = rpo.merge_device(level, children, 1 << (m - 1), empty(1 << (m - 1), d))
        assert torch.equal(t_nodes[(1 << (m - 1)) - 1:(1 << m) - 1], parents), m
    nodes_h = host(t_nodes)
    assert_canonical(nodes_h)
    assert np.array_equal(nodes_h[0], root)
    assert nodes_h[n - 1 + 5].tolist() == R.hash(level, [int(v) for v in cols[:, G.bitrev(5, log2n)]])
    # (b) the host form
    root_h, nodes_host = rpo.commit_columns(level, cols, True, return_nodes=True)
    assert np.array_equal(root_h, root) and np.array_equal(nodes_host, nodes_h)
    assert np.array_equal(rpo.commit_columns(level, cols, True), root)
    # (c) authentication paths through the existing call: 32-byte nodes, so the 128-bit level only
    if level != rpo.LEVEL_128:
        return
    positions = [0, n - 1] + [int(x) for x in np.random.default_rng(78).integers(0, n, 6)]
    tree = merkle.Tree(fft.Stark252PrimeField, t_nodes, log2n)
    _, paths = merkle.open_trees_device([tree], np.array(positions, np.uint64))
    assert paths[0].shape == (len(positions), log2n, 32)
    for q, pos in enumerate(positions):
        cur = R.hash(level, [int(v) for v in cols[:, G.bitrev(pos, log2n)]])
        assert cur == nodes_h[n - 1 + pos].tolist()
        i = pos
        for sib in paths[0][q].view(np.uint64).reshape(log2n, 4).tolist():
            cur = R.hash(level, cur + sib) if i % 2 == 0 else R.hash(level, sib + cur)
            i >>= 1
        assert cur == root.tolist(), pos


# ---- 6. LDE -> commit on the resident output
@pytest.mark.parametrize("level", LEVELS)
def test_lde_then_commit_resident(level):
    n_cols, log2c, log2n = 4, 8, 10
    coeffs = rand_words((n_cols, 1 << log2c), 91)
    t_lde = empty(n_cols, 1 << log2n)
    goldilocks.lde_device(dev(coeffs), log2c, t_lde, log2n, batch=n_cols, offset=7)
    t_nodes = empty(2 * (1 << log2n) - 1, rpo.digest_len(level))
    root = rpo.commit_columns_device(level, t_lde, n_cols, log2n, t_nodes, True)
    lde_ref = np.array([G.lde([int(v) for v in row], log2n, 7) for row in coeffs], np.uint64)
    assert np.array_equal(host(t_lde), lde_ref)
    exp = R.np_tree(level, lde_ref, True)
    assert np.array_equal(root, exp[0])
    assert np.array_equal(host(t_nodes), exp)


# ---- 7. misaligned device pointers and bad levels are rejected before any launch
def test_misaligned_device_pointers_and_levels():
    lib = L.lib()
    t = torch.zeros(1024, dtype=torch.int64, device="cuda")
    ok, off = t.data_ptr(), t.data_ptr() + 8
    assert ok % 16 == 0
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    BAD = L.ERR_BAD_ARG
    for level in (0, 1):
        for a, b in ((off, ok + 4096), (ok, off + 4096)):
            assert lib.lw_rpo_permute_device(level, a, 1, b, s) == BAD
            assert lib.lw_rpo_hash_device(level, a, 1, 2, 0, b, s) == BAD
            assert lib.lw_rpo_commit_columns_device(level, a, 1, 0, 2, 0, b, None, s) == BAD
    for level in (-1, 2):
        assert lib.lw_rpo_permute_device(level, ok, 1, ok + 4096, s) == BAD
        assert lib.lw_rpo_hash_device(level, ok, 1, 2, 0, ok + 4096, s) == BAD
        assert lib.lw_rpo_commit_columns_device(level, ok, 1, 0, 2, 0, ok + 4096, None, s) == BAD
    torch.cuda.synchronize()
    assert not t.any()
