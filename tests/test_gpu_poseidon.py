"""Starknet Poseidon on the device (csrc/poseidon.cuh, poseidon.hip) against the reference's fixed vectors
(tests/golden/poseidon_starknet.json) and the big-integer model (tests/poseidon_ref.py, about 2 600 permutations/s: every
case below keeps its model work to a few thousand permutations).

Launch boundaries of the tree (poseidon_commit_device): a workgroup is 256 work-items; the top kernel builds everything
from a level of 2^9 nodes (256 parents) down; every level above is one launch.  log2n = 9 and 10 straddle that boundary,
2^17 lies past it with 8 per-level launches."""
import ctypes as C
import itertools
import json
import os

import numpy as np
import pytest
import torch

from lambda_elliptic_curves_amd import _lib as L
from lambda_elliptic_curves_amd import fft, merkle, poseidon
from tests import poseidon_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BATCH, LANES = 257, (0, 63, 64, 256)   # a second workgroup, a partial last wave, not a multiple of 64


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint64).view(np.int64)).cuda()


def host(t):
    return t.cpu().numpy().view(np.uint64)


def empty(n):
    return torch.zeros((n, 4), dtype=torch.int64, device="cuda")


def rand_ints(n, seed):
    rng = np.random.default_rng(seed)
    return [int.from_bytes(rng.bytes(32), "little") % R.P for _ in range(n)]


def h(s):
    return int(s, 16)


def assert_canonical(elems):
    assert all(m < R.P for m in R.raw_ints(elems)), "a stored value is not below p"


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(ROOT, "tests", "golden", "poseidon_starknet.json")) as f:
        return json.load(f)


def placed(n_per, case_vals, seed):
    """a batch of BATCH inputs of n_per elements each: random, with the case at every lane of LANES"""
    vals = rand_ints(BATCH * n_per, seed)
    for lane in LANES:
        vals[lane * n_per:(lane + 1) * n_per] = case_vals
    return R.to_elems(vals)


# ---- 1. the reference's fixed vectors through the host and the _device forms
def test_kats_through_the_abi(golden):
    for c in golden["permutation"]:
        s = placed(3, [h(x) for x in c["state"]], 1).reshape(BATCH, 3, 4)
        exp = [h(x) for x in c["expected"]]
        got_h = poseidon.permute(s)
        t = dev(s)
        got_d = host(poseidon.permute_device(t, BATCH, torch.zeros_like(t)))
        for lane in LANES:
            assert R.from_elems(got_h[lane]) == exp and R.from_elems(got_d[lane]) == exp, (c["cite"], lane)
        assert np.array_equal(got_h, got_d)
    for c in golden["hash"]:
        x, y, exp = placed(1, [h(c["x"])], 2), placed(1, [h(c["y"])], 3), [h(c["expected"])]
        got_h = poseidon.hash(x, y)
        got_d = host(poseidon.hash_device(dev(x), dev(y), BATCH, empty(BATCH)))
        for lane in LANES:
            assert R.from_elems(got_h[lane]) == exp and R.from_elems(got_d[lane]) == exp, (c["cite"], lane)
        assert np.array_equal(got_h, got_d)
    for c in golden["hash_single"]:
        x, exp = placed(1, [h(c["x"])], 4), [h(c["expected"])]
        got_h = poseidon.hash_single(x)
        got_d = host(poseidon.hash_single_device(dev(x), BATCH, empty(BATCH)))
        for lane in LANES:
            assert R.from_elems(got_h[lane]) == exp and R.from_elems(got_d[lane]) == exp, (c["cite"], lane)
        assert np.array_equal(got_h, got_d)
    for k, c in enumerate(golden["hash_many"]):
        ins, exp = [h(x) for x in c["inputs"]], [h(c["expected"])]
        rows = placed(len(ins), ins, 5 + k).reshape(BATCH, len(ins), 4)
        got_h = poseidon.hash_many(rows)
        got_d = host(poseidon.hash_many_device(dev(rows), BATCH, len(ins), empty(BATCH)))
        for lane in LANES:
            assert R.from_elems(got_h[lane]) == exp and R.from_elems(got_d[lane]) == exp, (c["cite"], lane)
        assert np.array_equal(got_h, got_d)


# ---- 2. edge operands: the stored (Montgomery-form) words themselves are the edge values
def raw_to_elems(raws):
    out = np.zeros((len(raws), 4), np.uint64)
    for i, m in enumerate(raws):
        for k in range(4):
            out[i, 3 - k] = (m >> (64 * k)) & 0xffffffffffffffff
    return out


def test_edge_operands_exact_and_canonical():
    ones_low = (0x0800000000000010 << 192) | ((1 << 192) - 1)   # the largest top limb below p's with all-ones low limbs
    edges = [0, 1, R.P - 1, R.P - 2, R.R % R.P, (1 << 251) - 1, ones_low, (1 << 192) - 1]
    assert all(e < R.P for e in edges)
    raws = [w for st in itertools.product(edges, edges, [0, R.P - 1, R.R % R.P, ones_low]) for w in st]
    assert len(raws) == 256 * 3
    s = raw_to_elems(raws).reshape(256, 3, 4)
    canon = [m * R.R_INV % R.P for m in raws]
    exp = [w for i in range(256) for w in R.permute(canon[3 * i:3 * i + 3])]
    t = dev(s)
    out = host(poseidon.permute_device(t, 256, torch.zeros_like(t)))
    assert_canonical(out)
    assert R.from_elems(out) == exp
    inplace = host(poseidon.permute_device(t, 256))   # out == states
    assert np.array_equal(inplace, out)
    assert np.array_equal(poseidon.permute(s), out)


# ---- 3. random parity
def test_random_permute_and_hash():
    n = 1000
    vals = rand_ints(3 * n, 11)
    out = host(poseidon.permute_device(dev(R.to_elems(vals).reshape(n, 3, 4)), n))
    assert_canonical(out)
    assert R.from_elems(out) == [w for i in range(n) for w in R.permute(vals[3 * i:3 * i + 3])]
    xs, ys = rand_ints(n, 12), rand_ints(n, 13)
    out = host(poseidon.hash_device(dev(R.to_elems(xs)), dev(R.to_elems(ys)), n, empty(n)))
    assert_canonical(out)
    assert R.from_elems(out) == [R.hash2(x, y) for x, y in zip(xs, ys)]


@pytest.mark.parametrize("row_len", [0, 1, 2, 3, 4, 7, 8])   # odd and even: both padding branches; 0: the padding alone
def test_random_hash_many(row_len):
    n = 65
    vals = rand_ints(n * row_len, 20 + row_len)
    exp = [R.hash_many(vals[i * row_len:(i + 1) * row_len]) for i in range(n)]
    rows = R.to_elems(vals).reshape(n, row_len, 4)
    t_rows = dev(rows) if row_len else torch.zeros((1, 4), dtype=torch.int64, device="cuda")
    out = host(poseidon.hash_many_device(t_rows, n, row_len, empty(n)))
    assert_canonical(out)
    assert R.from_elems(out) == exp
    assert np.array_equal(poseidon.hash_many(rows), out)
    if row_len == 1:   # hash_many of one element is not hash_single of it
        assert not np.array_equal(poseidon.hash_single(rows.reshape(n, 4)), out)


# ---- 4. small trees, every node against the model
def device_tree(cols, leaf_mode, bit_reverse, stride=0):
    n_cols, n = cols.shape[0], cols.shape[1]
    if stride:
        padded = np.zeros((n_cols, stride, 4), np.uint64)
        padded[:, n:] = np.uint64(0xdeadbeefdeadbeef)   # between the columns: never read
        padded[:, :n] = cols
        cols = padded
    t_nodes = empty(2 * n - 1)
    root = poseidon.commit_columns_device(dev(cols), n_cols, n.bit_length() - 1, t_nodes, leaf_mode, bit_reverse, col_stride_elems=stride)
    nodes = host(t_nodes)
    assert np.array_equal(root, nodes[0])
    return nodes


TREES = [(poseidon.LEAF_SINGLE, 1, k) for k in (0, 1, 2, 9, 10)] + [(poseidon.LEAF_MANY, c, k) for c, k in ((1, 3), (2, 3), (3, 10), (5, 6))]


@pytest.mark.parametrize("bit_reverse", [True, False])
@pytest.mark.parametrize("leaf_mode,n_cols,log2n", TREES)
def test_small_trees_every_node(leaf_mode, n_cols, log2n, bit_reverse):
    n = 1 << log2n
    vals = rand_ints(n_cols * n, 100 + 16 * n_cols + log2n)
    columns = [vals[c * n:(c + 1) * n] for c in range(n_cols)]
    exp = R.commit_columns(columns, leaf_mode == poseidon.LEAF_MANY, bit_reverse)
    nodes = device_tree(R.to_elems(vals).reshape(n_cols, n, 4), leaf_mode, bit_reverse)
    assert_canonical(nodes)
    assert R.from_elems(nodes) == exp


def test_tree_with_a_column_stride():
    n_cols, log2n = 2, 3
    n = 1 << log2n
    vals = rand_ints(n_cols * n, 7)
    exp = R.commit_columns([vals[:n], vals[n:]], True, True)
    nodes = device_tree(R.to_elems(vals).reshape(n_cols, n, 4), poseidon.LEAF_MANY, True, stride=n + 5)
    assert R.from_elems(nodes) == exp


def test_one_column_leaf_many_is_not_leaf_single():
    vals = rand_ints(8, 9)
    col = R.to_elems(vals).reshape(1, 8, 4)
    many, single = device_tree(col, poseidon.LEAF_MANY, False), device_tree(col, poseidon.LEAF_SINGLE, False)
    assert R.from_elems(many[7:]) == [R.hash_many([v]) for v in vals]
    assert R.from_elems(single[7:]) == [R.hash_single(v) for v in vals]
    assert not np.array_equal(many[7:], single[7:]) and not np.array_equal(many[0], single[0])


# ---- 5. a tree past every launch threshold: 2^17 leaves, 8 per-level launches and the top kernel
def test_large_tree_levels_and_openings():
    log2n = 17
    n = 1 << log2n
    rng = np.random.default_rng(17)
    col = rng.integers(0, 1 << 63, size=(n, 4), dtype=np.uint64)
    col[:, 0] &= np.uint64(0x07ffffffffffffff)   # below 2^251 < p: canonical stored values
    t_col, t_nodes = dev(col), empty(2 * n - 1)
    root = poseidon.commit_columns_device(t_col, 1, log2n, t_nodes, poseidon.LEAF_SINGLE, True)
    # (a) every level from the level below with the flat calls (tied to the model by the tests above)
    perm = torch.tensor([R.bitrev(i, log2n) for i in range(n)], dtype=torch.int64, device="cuda")
    leaves = poseidon.hash_single_device(t_col, n, empty(n))[perm]
    assert torch.equal(t_nodes[n - 1:], leaves)
    for m in range(log2n, 0, -1):
        level = t_nodes[(1 << m) - 1:(1 << (m + 1)) - 1]
        left, right = level[0::2].contiguous(), level[1::2].contiguous()
        parents = poseidon.hash_device(left, right, 1 << (m - 1), empty(1 << (m - 1)))
        assert torch.equal(t_nodes[(1 << (m - 1)) - 1:(1 << m) - 1], parents), m
    assert np.array_equal(host(t_nodes[0:1])[0], root)
    # (b) openings through the existing call, folded up to the device's root with the model
    positions = [0, n - 1] + [int(x) for x in np.random.default_rng(18).integers(0, n, 64)]
    tree = merkle.Tree(fft.Stark252PrimeField, t_nodes, log2n)
    _, paths = merkle.open_trees_device([tree], np.array(positions, np.uint64))
    assert paths[0].shape == (len(positions), log2n, 32)
    nodes_h = host(t_nodes)
    root_int = R.from_elems(root)[0]
    for q, pos in enumerate(positions):
        value = R.from_elems(col[R.bitrev(pos, log2n)])[0]
        cur = R.hash_single(value)
        assert cur == R.from_elems(nodes_h[n - 1 + pos])[0]
        i = pos
        for sib in R.from_elems(paths[0][q].view(np.uint64)):
            cur = R.hash2(cur, sib) if i % 2 == 0 else R.hash2(sib, cur)
            i >>= 1
        assert cur == root_int, pos


# ---- 6. host form = device form
def test_commit_host_form_equals_device_form():
    n_cols, log2n = 3, 10
    n = 1 << log2n
    cols = R.to_elems(rand_ints(n_cols * n, 31)).reshape(n_cols, n, 4)
    nodes_d = device_tree(cols, poseidon.LEAF_MANY, True)
    root, nodes_h = poseidon.commit_columns(cols, poseidon.LEAF_MANY, True, return_nodes=True)
    assert np.array_equal(nodes_h, nodes_d) and np.array_equal(root, nodes_d[0])
    assert np.array_equal(poseidon.commit_columns(cols, poseidon.LEAF_MANY, True), root)


# ---- 7. misaligned device pointers are rejected before any launch
def test_misaligned_device_pointers():
    lib = L.lib()
    t = torch.zeros((64, 4), dtype=torch.int64, device="cuda")
    ok, off = t.data_ptr(), t.data_ptr() + 8
    assert ok % 16 == 0
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    BAD = L.ERR_BAD_ARG
    for a, b in ((off, ok), (ok, off)):
        assert lib.lw_poseidon_permute_device(a, 1, b, s) == BAD
        assert lib.lw_poseidon_hash_single_device(a, 1, b, s) == BAD
        assert lib.lw_poseidon_hash_many_device(a, 1, 2, b, s) == BAD
        assert lib.lw_poseidon_commit_columns_device(a, 1, 0, 2, 0, L.POSEIDON_LEAF_MANY, b, None, s) == BAD
    for a, b, c in ((off, ok, ok), (ok, off, ok), (ok, ok, off)):
        assert lib.lw_poseidon_hash_device(a, b, 1, c, s) == BAD
    torch.cuda.synchronize()
    assert not t.any()
