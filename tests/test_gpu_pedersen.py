"""Starknet Pedersen hash on the device (csrc/pedersen.cuh, pedersen.hip) against the recorded vectors
(tests/golden/pedersen_starkcurve.json) and the big-integer model (tests/pedersen_ref.py, about 2 000 hashes/s: every
case below keeps its model work under 1 500 hashes, and the random batch is hashed by the model once for all of them).

The branches of the group law that no hash input reaches (doubling, opposite points, the point at infinity) run through
pedersen.add_affine_device, which calls the hash kernel's own addition and normalisation.

Launch boundaries of the tree (hash_tree.cuh tree_commit_device): a workgroup is 256 work-items; the top kernel builds
everything from a level of 2^9 nodes down; every level above is one launch.  log2n = 9 and 10 straddle that boundary."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from lambda_elliptic_curves_amd import fft, merkle, pedersen
from tests import pedersen_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BATCH, LANES = 257, (0, 63, 64, 256)   # a second workgroup, a partial last wave, not a multiple of 64


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint64).view(np.int64)).cuda()


def host(t):
    return t.cpu().numpy().view(np.uint64)


def empty(*shape):
    return torch.zeros(shape + (4,), dtype=torch.int64, device="cuda")


def rand_ints(n, seed):
    rng = np.random.default_rng(seed)
    return [int.from_bytes(rng.bytes(32), "little") % R.P for _ in range(n)]


def h(s):
    return int(s, 16)


def assert_canonical(elems):
    assert all(m < R.P for m in R.raw_ints(elems)), "a stored value is not below p"


with open(os.path.join(ROOT, "tests", "golden", "pedersen_starkcurve.json")) as _f:
    GOLDEN = json.load(_f)
V = 0x03a5c1f2e4b6d8790123456789abcdef0fedcba987654321f0e1d2c3b4a59687 % R.P   # an arbitrary partner value
EDGES = [(h(c["x"]), h(c["y"])) for c in GOLDEN["hash"]]                           # the reference's vector, (0, 0), (p-1, p-1)
for _side in (0, 1):
    for _e in ((1 << 248) - 1,                     # every low nibble 15, nothing from T2 (T4)
               1 << 248, 1 << 251,                 # entries 0 and 7 of T2 (T4) alone
               1, 1 << (4 * 31), 1 << (4 * 61),    # one entry of row 0, 31 and 61 of T1 (T3)
               0):                                 # (0, v) and (v, 0): one side contributes nothing
        EDGES.append((_e, V) if _side == 0 else (V, _e))
assert len(EDGES) == 17


@pytest.fixture(scope="module")
def random_batch():
    """BATCH random pairs and their model hashes, computed once; the tests copy and never change them"""
    xs, ys = rand_ints(BATCH, 1), rand_ints(BATCH, 2)
    return xs, ys, [R.hash(x, y) for x, y in zip(xs, ys)]


# ---- 1. hashes: host and device forms, bit-exact, canonical
def test_golden_expected_values_through_both_forms():
    xs = [h(c["x"]) for c in GOLDEN["hash"]]
    ys = [h(c["y"]) for c in GOLDEN["hash"]]
    exp = [h(c["expected"]) for c in GOLDEN["hash"]]
    x, y = R.to_elems(xs), R.to_elems(ys)
    assert R.from_elems(pedersen.hash(x, y)) == exp
    assert R.from_elems(host(pedersen.hash_device(dev(x), dev(y), len(xs), empty(len(xs))))) == exp


@pytest.mark.parametrize("case", range(len(EDGES)))
def test_edge_inputs_at_the_wave_and_workgroup_boundaries(case, random_batch):
    xs, ys, exp = (list(v) for v in random_batch)
    ex, ey = EDGES[case]
    eh = R.hash(ex, ey)
    for lane in LANES:
        xs[lane], ys[lane], exp[lane] = ex, ey, eh
    x, y = R.to_elems(xs), R.to_elems(ys)
    got_h = pedersen.hash(x, y)
    got_d = host(pedersen.hash_device(dev(x), dev(y), BATCH, empty(BATCH)))
    assert_canonical(got_h)
    assert R.from_elems(got_h) == exp
    assert np.array_equal(got_h, got_d)


@pytest.mark.parametrize("n", [1, 64, 65, 257])
def test_batch_sizes(n, random_batch):
    xs, ys, exp = random_batch
    x, y = R.to_elems(xs[:n]), R.to_elems(ys[:n])
    out = torch.full((n + 1, 4), -1, dtype=torch.int64, device="cuda")
    got_d = host(pedersen.hash_device(dev(x), dev(y), n, out))
    assert R.from_elems(got_d[:n]) == exp[:n]
    assert (got_d[n] == np.uint64(0xffffffffffffffff)).all(), "written past the batch"
    assert np.array_equal(pedersen.hash(x, y), got_d[:n])


# ---- 2. the group law through the seam: every branch, Z != 1
def seam_rows():
    t = R.tables()
    rng = np.random.default_rng(5)
    pick = lambda: t[int(rng.integers(0, len(t)))]
    by_y, by_x = sorted(t, key=lambda pt: pt[1]), sorted(t, key=lambda pt: pt[0])
    # the table's points nearest to the ends of the field in either coordinate (y nearest p - 1 and 0, x likewise)
    extreme = [by_y[-1], by_y[-2], by_y[0], by_x[-1], by_x[0]]
    rows = []
    for _ in range(8):
        rows.append((pick(), pick()))                      # generic P + Q
    for _ in range(4):
        q = pick()
        rows += [(q, q), (q, R.neg(q)), (R.neg(q), q), (None, q)]   # doubling, infinity out, infinity in
    rows.append((R.P0, t[0]))                              # the first addition of most hashes
    for a in extreme:
        rows += [(a, a), (a, R.neg(a)), (None, a), (a, R.P0), (R.P0, a)]
        rows += [(a, b) for b in extreme if b != a]
    return rows


@pytest.mark.parametrize("z_kind", ["one", "two", "p-1", "random"])
def test_group_law_through_the_seam(z_kind):
    rows = seam_rows()
    n = len(rows)
    assert n > 64 and any(p == q for p, q in rows) and any(p is None for p, _ in rows)
    zs = {"one": [1] * n, "two": [2] * n, "p-1": [R.P - 1] * n, "random": [z or 1 for z in rand_ints(n, 6)]}[z_kind]
    exp = [R.add(p, q) for p, q in rows]
    assert sum(e is None for e in exp) >= 9 and all(R.on_curve(e) for e in exp)
    t_p, t_q = dev(R.points_to_elems([p for p, _ in rows])), dev(R.points_to_elems([q for _, q in rows]))
    out = host(pedersen.add_affine_device(t_p, dev(R.to_elems(zs)), t_q, n, empty(n, 2)))
    assert_canonical(out)
    got = R.points_from_elems(out)
    bad = [i for i in range(n) if got[i] != exp[i]]
    assert not bad, f"rows {bad} differ from the model"
    assert not out[[i for i in range(n) if exp[i] is None]].any()   # infinity is written as (0, 0) exactly


# ---- 3. the tree over leaf values
def device_tree(leaves, bit_reverse):
    n = leaves.shape[0]
    t_nodes = empty(2 * n - 1)
    root = pedersen.commit_leaves_device(dev(leaves), n.bit_length() - 1, t_nodes, bit_reverse)
    nodes = host(t_nodes)
    assert np.array_equal(root, nodes[0])
    return t_nodes, nodes


@pytest.mark.parametrize("bit_reverse", [True, False])
@pytest.mark.parametrize("log2n", [0, 1, 9, 10])
def test_trees_every_node(log2n, bit_reverse):
    n = 1 << log2n
    vals = rand_ints(n, 100 + log2n)
    exp = R.commit_leaves(vals, bit_reverse)
    leaves = R.to_elems(vals)
    root, nodes = pedersen.commit_leaves(leaves, bit_reverse, return_nodes=True)   # host form, all nodes
    assert_canonical(nodes)
    assert R.from_elems(nodes) == exp
    assert np.array_equal(root, nodes[0])
    assert np.array_equal(pedersen.commit_leaves(leaves, bit_reverse), root)       # host form, root only
    _, nodes_d = device_tree(leaves, bit_reverse)                                  # device form
    assert np.array_equal(nodes_d[0], root) and np.array_equal(nodes_d, nodes)


def test_an_opening_folds_up_to_the_root():
    log2n = 6
    n = 1 << log2n
    vals = rand_ints(n, 9)
    t_nodes, nodes = device_tree(R.to_elems(vals), True)
    root_int = R.from_elems(nodes[0])[0]
    positions = [0, 37, n - 1]
    tree = merkle.Tree(fft.Stark252PrimeField, t_nodes, log2n)
    _, paths = merkle.open_trees_device([tree], np.array(positions, np.uint64))
    assert paths[0].shape == (len(positions), log2n, 32)
    for q, pos in enumerate(positions):
        cur = vals[R.bitrev(pos, log2n)]   # identity leaves: the node is the value
        assert cur == R.from_elems(nodes[n - 1 + pos])[0]
        i = pos
        for sib in R.from_elems(paths[0][q].view(np.uint64)):
            cur = R.hash(cur, sib) if i % 2 == 0 else R.hash(sib, cur)
            i >>= 1
        assert cur == root_int, pos


FIRST_CALL = """
import sys, numpy as np, torch
from lambda_elliptic_curves_amd import pedersen
leaves = np.frombuffer(bytes.fromhex(sys.argv[1]), np.int64).reshape(8, 4)
t_nodes = torch.zeros((15, 4), dtype=torch.int64, device="cuda")
pedersen.commit_leaves_device(torch.from_numpy(leaves.copy()).cuda(), 3, t_nodes)
print(t_nodes.cpu().numpy().tobytes().hex())
"""


def test_the_first_call_of_a_process_may_be_a_device_tree():
    """The lookup table is uploaded inside the tree call (PedersenHash::ready), under the call's one hold of the lane: a
    process whose first library call is commit_leaves_device gets all 15 nodes right.  A tree built against a table that
    is not there hashes against zeros."""
    vals = rand_ints(8, 77)
    out = subprocess.run([sys.executable] + (["-s"] if sys.flags.no_user_site else []) + ["-c", FIRST_CALL, R.to_elems(vals).tobytes().hex()],
                         cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    nodes = np.frombuffer(bytes.fromhex(out.stdout.split()[-1]), np.uint64).reshape(15, 4)
    assert R.from_elems(nodes) == R.commit_leaves(vals, True)


def test_two_columns_are_refused():
    from lambda_elliptic_curves_amd import errors
    t = empty(8)
    with pytest.raises(errors.HipError):
        pedersen.commit_leaves_device(t, 2, empty(7), n_cols=2)
    torch.cuda.synchronize()
