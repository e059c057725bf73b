"""STARK round 4 tail on the device (stark_query.hip): the grinding nonce search against the fixture's smallest nonces and
the CPU restatement, and the query openings against the restatement run on host copies of the same trees."""
import hashlib
import json
import os
import time

import numpy as np
import pytest

from oracle import oracle as O
from tests import stark_query_ref as R
from tests import util
from tests.test_stark_query_cpu import stone_case_1_opening

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALLEST_B_20 = 0x2c5db8


@pytest.fixture(scope="module")
def grinding():
    with open(os.path.join(ROOT, "tests", "golden", "stark_grinding.json")) as f:
        g = json.load(f)
    g["seeds"] = {k: bytes(v) for k, v in g["seeds"].items()}
    return g


def cuda(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).cuda()


# ---- grinding

def test_every_smallest_nonce_of_the_fixture(grinding):
    from lambda_elliptic_curves_amd import stark
    for name, row in grinding["smallest"].items():
        for g, nonce in row.items():
            assert stark.grinding_nonce(grinding["seeds"][name], int(g)) == int(nonce, 16), (name, g)


def test_search_from_the_middle_returns_the_next_valid_nonce(grinding):
    from lambda_elliptic_curves_amd import stark
    for name, row in grinding["smallest"].items():
        for g, nonce in row.items():
            g, nonce, seed = int(g), int(nonce, 16), grinding["seeds"][name]
            if g > 10:
                continue
            nxt = stark.grinding_nonce(seed, g, first=nonce + 1)
            assert nxt is not None and nxt > nonce and R.is_valid_nonce(seed, nxt, g), (name, g)
            inner = R.inner_hash(seed, g)
            assert not any(R.is_valid_nonce(seed, c, g, inner) for c in range(nonce + 1, nxt)), (name, g)
            # the device form on a stream of the caller's gives the same answer
            import torch
            assert stark.grinding_nonce(seed, g, first=nonce + 1, stream=torch.cuda.current_stream().cuda_stream) == nxt


def test_range_ends_at_factor_20(grinding):
    from lambda_elliptic_curves_amd import stark
    seed = grinding["seeds"]["B"]
    assert stark.grinding_nonce(seed, 20, last=SMALLEST_B_20 - 1) is None
    assert stark.grinding_nonce(seed, 20, last=SMALLEST_B_20) == SMALLEST_B_20
    assert stark.grinding_nonce(seed, 20, first=SMALLEST_B_20, last=SMALLEST_B_20) == SMALLEST_B_20


def test_hit_at_the_last_and_at_the_first_candidate_of_a_window(grinding):
    from lambda_elliptic_curves_amd import stark
    seed, w = grinding["seeds"]["B"], stark.grinding_window(20)
    assert 0 < w <= SMALLEST_B_20       # no valid nonce lies below SMALLEST_B_20, so `first` alone places it in its window
    assert stark.grinding_nonce(seed, 20, first=SMALLEST_B_20 - w + 1) == SMALLEST_B_20     # last candidate of window 0
    assert stark.grinding_nonce(seed, 20, first=SMALLEST_B_20 - w) == SMALLEST_B_20         # first candidate of window 1
    assert stark.grinding_nonce(seed, 20, first=SMALLEST_B_20 - w + 1, last=SMALLEST_B_20 - 1) is None


@pytest.mark.parametrize("g", [30, 33])
def test_reference_vectors_at_factor_30_and_33(grinding, g):
    """The reference's valid vectors (grinding.rs:142-167); nobody has shown them to be the smallest, so the device's answer
    must be valid and not above them.  Time limit: ten times what the rate of a search at factor 20 predicts, plus a
    second, checked between calls of at most 2^28 candidates."""
    from lambda_elliptic_curves_amd import stark
    seed = grinding["seeds"]["B"]
    vector = next(int(v["nonce"], 16) for v in grinding["valid"] if v["grinding_factor"] == g)
    stark.grinding_nonce(seed, 20, last=SMALLEST_B_20 - 1)   # warm-up
    t0 = time.perf_counter()
    assert stark.grinding_nonce(seed, 20, last=SMALLEST_B_20 - 1) is None
    rate = SMALLEST_B_20 / (time.perf_counter() - t0)
    limit = 10.0 * (vector + 1) / rate + 1.0
    print(f"factor 20: {rate / 1e9:.3f} G candidates/s over {SMALLEST_B_20} candidates; limit for factor {g}: {limit:.2f} s")
    got, first, t0 = None, 0, time.perf_counter()
    while got is None and first <= vector:
        last = min(vector, first + (1 << 28) - 1)
        got = stark.grinding_nonce(seed, g, first=first, last=last)
        first = last + 1
        elapsed = time.perf_counter() - t0
        assert elapsed < limit, f"factor {g}: {elapsed:.2f} s for {first} candidates, limit {limit:.2f} s"
    print(f"factor {g}: device {got:#x}, reference vector {vector:#x}, equal: {got == vector}, {elapsed:.3f} s")
    assert got is not None and got <= vector and R.is_valid_nonce(seed, got, g)


# ---- grinding at nonces of the full width: v = bswap64(nonce) has a low half that is not zero from 2^32 on

def test_pointwise_validity_at_full_width_nonces(grinding):
    """first == last == nonce makes the search the predicate: one launch of one candidate per (seed, factor, nonce)"""
    from lambda_elliptic_curves_amd import stark
    nonces = [int(x, 16) for x in grinding["pointwise"]["nonces"]]
    assert nonces == R.pointwise_nonces()
    n_calls, wrong = 0, []
    for name, rows in grinding["pointwise"]["valid"].items():
        seed = grinding["seeds"][name]
        for g in (1, 2, 3, 4):
            for nonce, bit in zip(nonces, rows[str(g)]):
                got = stark.grinding_nonce(seed, g, first=nonce, last=nonce)
                assert got in (None, nonce)
                n_calls += 1
                if (got == nonce) != (bit == "1"):
                    wrong.append((name, g, hex(nonce)))
    assert n_calls == 2 * 4 * 77
    assert not wrong, (len(wrong), wrong[:8])


def test_searches_above_two_to_the_32(grinding):
    """factor 8 over [first, first + 5000] from 2^32, 2^40 + 12345, 2^63 and 2^64 - 2^20, the ranges that end at 2^64 - 2 at
    factors 8 and 20 (a hit or None, as the restatement says), on the library's stream and on the caller's"""
    import torch
    from lambda_elliptic_curves_amd import stark
    own = torch.cuda.current_stream().cuda_stream
    seen = set()
    for s in grinding["searches"]:
        seed, g, first, last = grinding["seeds"][s["seed"]], s["grinding_factor"], int(s["first"], 16), int(s["last"], 16)
        want = None if s["nonce"] is None else int(s["nonce"], 16)
        assert stark.grinding_nonce(seed, g, first=first, last=last) == want, s
        assert stark.grinding_nonce(seed, g, first=first, last=last, stream=own) == want, s
        seen.add((g, want is None))
    assert {(8, False), (20, True), (1, False)} <= seen


def test_the_largest_u64_is_never_a_candidate(grinding):
    """grinding.rs:45 iterates 0..u64::MAX: last = 2^64 - 1 means 2^64 - 2, and [2^64 - 1, 2^64 - 1] holds nothing, although
    the restatement finds 2^64 - 1 valid for seed B at factor 1"""
    import torch
    from lambda_elliptic_curves_amd import stark
    seed, top = grinding["seeds"]["B"], 2**64 - 1
    assert R.is_valid_nonce(seed, top, 1) and R.is_valid_nonce(seed, top - 1, 1)
    for stream in (None, torch.cuda.current_stream().cuda_stream):
        assert stark.grinding_nonce(seed, 1, first=top, last=top, stream=stream) is None
        assert stark.grinding_nonce(seed, 1, first=top - 1, stream=stream) == top - 1
        assert stark.grinding_nonce(seed, 1, first=top - 1, last=top - 1, stream=stream) == top - 1
    for s in grinding["searches"]:              # a range that ends at 2^64 - 1 is the range that ends at 2^64 - 2
        if int(s["last"], 16) == top - 1 and s["grinding_factor"] == 8:
            want = int(s["nonce"], 16)
            assert stark.grinding_nonce(grinding["seeds"][s["seed"]], 8, first=int(s["first"], 16), last=top) == want
            assert stark.grinding_nonce(grinding["seeds"][s["seed"]], 8, first=int(s["first"], 16)) == want


def test_two_windows_that_end_at_the_top_of_the_range(grinding):
    """factor 63 over [2^64 - 2^28 - 3, 2^64 - 1]: a full window of 2^28 candidates, then the rest up to 2^64 - 2, whose
    start + window - 1 would wrap.  None: a candidate is valid with probability 2^-63.  The time limit is ten times what
    the rate of a search at factor 20 predicts for 2^28 candidates, plus a second."""
    from lambda_elliptic_curves_amd import stark
    seed, w = grinding["seeds"]["A"], stark.grinding_window(63)
    first = 2**64 - w - 3
    assert w == 1 << 28 and first + w - 1 < 2**64 - 2 < first + 2 * w - 1
    stark.grinding_nonce(grinding["seeds"]["B"], 20, last=SMALLEST_B_20 - 1)   # warm-up
    t0 = time.perf_counter()
    assert stark.grinding_nonce(grinding["seeds"]["B"], 20, last=SMALLEST_B_20 - 1) is None
    rate = SMALLEST_B_20 / (time.perf_counter() - t0)
    limit = 10.0 * (w + 2) / rate + 1.0
    t0 = time.perf_counter()
    got = stark.grinding_nonce(seed, 63, first=first, last=2**64 - 1)
    elapsed = time.perf_counter() - t0
    print(f"factor 63: {w + 2} candidates in {elapsed:.3f} s, limit {limit:.2f} s")
    assert got is None
    assert elapsed < limit


# ---- openings

def _positions(leaves):
    """0, the last leaf, a duplicate, and both children of one parent"""
    pair = 2 * (leaves // 4)
    return [0, leaves - 1, leaves - 1, pair, min(pair + 1, leaves - 1)]


@pytest.fixture(scope="module")
def tree_cases():
    """Per field every (log2_rows, n_cols, rows_per_leaf, bit_reverse) shape; every third tree with a non-dense stride.
    nodes: the device commitment where lw_stark_commit_columns_device makes that shape (one row per leaf, dense), random
    bytes elsewhere (a path depends on `nodes` alone).  -> {field name: [(merkle.Tree, host columns, host nodes)]}"""
    import torch
    from lambda_elliptic_curves_amd import merkle
    rng = np.random.default_rng(11)
    out = {}
    for name, (fld, _oid) in util.field_pairs().items():
        if name not in ("stark252", "fr381"):
            continue
        cases, k = [], 0
        for log2_rows in range(7):
            for n_cols in (1, 3):
                for rpl in (1, 2):
                    for br in (False, True):
                        if log2_rows == 0 and rpl == 2:
                            continue
                        k += 1
                        rows = 1 << log2_rows
                        stride = rows + 3 if k % 3 == 0 else rows
                        host = util.rand_elems(name, n_cols * stride, 7000 + k).reshape(n_cols, stride, 4)
                        t_cols = cuda(host)
                        leaves = rows // rpl
                        if rpl == 1 and stride == rows:
                            t_nodes = torch.empty((2 * leaves - 1) * 4, dtype=torch.int64, device="cuda")
                            merkle.commit_columns_device(fld, t_cols, n_cols, log2_rows, t_nodes, bit_reverse=br)
                            nodes = t_nodes.cpu().numpy().view(np.uint8).reshape(-1, 32)
                        else:
                            nodes = rng.integers(0, 256, (2 * leaves - 1, 32), dtype=np.uint8)
                            t_nodes = cuda(nodes.view(np.uint64))
                        tree = merkle.Tree(fld, t_nodes, log2_rows, t_columns=t_cols, n_cols=n_cols, rows_per_leaf=rpl, bit_reverse=br,
                                           col_stride_elems=0 if stride == rows else stride)
                        cases.append((tree, host, nodes))
        out[name] = cases
    return out


def _check_tree(tree, host, nodes, pos, values, paths):
    for s, p in enumerate(pos):
        want_v, want_p = R.open_tree(host if values is not None else None, nodes, tree.log2_rows, tree.rows_per_leaf, tree.bit_reverse, int(p))
        assert paths[s].shape == want_p.shape and np.array_equal(paths[s], want_p)
        if values is not None:
            assert np.array_equal(values[s], want_v)


@pytest.mark.parametrize("name", ["stark252", "fr381"])
def test_all_shapes_in_one_call(tree_cases, name):
    from lambda_elliptic_curves_amd import merkle
    cases = tree_cases[name]
    pos = np.array([_positions(1 << t.log2_leaves) for t, _, _ in cases], np.uint64)
    values, paths = merkle.open_trees_device([t for t, _, _ in cases], pos)
    for k, (tree, host, nodes) in enumerate(cases):
        _check_tree(tree, host, nodes, pos[k], values[k], paths[k])


def test_one_tree_per_call_and_paths_only(tree_cases):
    from lambda_elliptic_curves_amd import merkle
    for tree, host, nodes in tree_cases["stark252"][::5]:
        pos = np.array([_positions(1 << tree.log2_leaves)], np.uint64)
        values, paths = merkle.open_trees_device([tree], pos)
        _check_tree(tree, host, nodes, pos[0], values[0], paths[0])
        bare = merkle.Tree(tree.field, tree.t_nodes, tree.log2_rows, rows_per_leaf=tree.rows_per_leaf, bit_reverse=tree.bit_reverse)
        values, paths2 = merkle.open_trees_device([bare, tree, bare], np.repeat(pos, 3, axis=0))
        assert values[0] is None and values[2] is None
        _check_tree(tree, host, nodes, pos[0], values[1], paths2[1])
        assert np.array_equal(paths2[0], paths[0]) and np.array_equal(paths2[2], paths[0])


def test_a_committed_path_folds_to_the_root(tree_cases):
    from lambda_elliptic_curves_amd import merkle
    done = 0
    for tree, host, nodes in tree_cases["stark252"]:
        if tree.rows_per_leaf != 1 or tree.col_stride_elems or tree.log2_rows < 3:
            continue
        leaves = 1 << tree.log2_rows
        pos = np.array([_positions(leaves)], np.uint64)
        values, paths = merkle.open_trees_device([tree], pos)
        for s, p in enumerate(pos[0]):
            leaf = O.keccak256(b"".join(values[0][s, 0, c].astype(">u8").tobytes() for c in range(tree.n_cols)))
            assert R.fold_path(leaf, int(p), paths[0][s]) == nodes[0].tobytes()
        done += 1
    assert done >= 4


def test_fri_query_phase_end_to_end():
    import torch
    from lambda_elliptic_curves_amd import fft, merkle, stark
    from oracle import bigint_def as D
    f, p, F = O.F_STARK252, D.P_STARK252, fft.Stark252PrimeField
    n, domain = 1 << 6, 1 << 8
    a = util.rand_elems("stark252", n, 4242)
    a[-1, -1] |= np.uint64(1)
    state = {"s": b"fri-query-test"}

    def sample_zeta():
        state["s"] = hashlib.sha256(state["s"] + b"z").digest()
        return O.elems_to_mont(f, [int.from_bytes(state["s"], "big") % p])[0]

    def append_root(root):
        state["s"] = hashlib.sha256(state["s"] + root).digest()

    _, layers = merkle.fri_commit_phase_device(F, 7, cuda(a), n, sample_zeta, append_root,
                                               lambda k: O.elems_to_mont(f, [pow(3, 1 << k, p)])[0], domain)
    assert [d for _, _, _, d in layers] == [128, 64, 32, 16, 8, 4]
    iotas = [0, domain // 2 - 1, 77, 77, 100]
    got = stark.fri_query_phase_device(F, layers, iotas)
    host = [(t_ev.cpu().numpy().view(np.uint64).reshape(-1, 4), t_nodes.cpu().numpy().view(np.uint8).reshape(-1, 32))
            for t_ev, t_nodes, _, _ in layers]
    want = R.fri_query_phase(host, iotas)
    assert len(got) == len(want) == len(iotas)
    for (g_sym, g_paths), (w_sym, w_paths), iota in zip(got, want, iotas):
        assert np.array_equal(g_sym, w_sym)
        assert len(g_paths) == len(w_paths) == len(layers)
        for k, (gp, wp) in enumerate(zip(g_paths, w_paths)):
            assert gp.shape == wp.shape and np.array_equal(gp, wp)
            # the leaf of (evaluation[index & ~1], evaluation[index | 1]) folds to the root the transcript absorbed
            ev, index = host[k][0], iota >> k
            leaf = O.keccak256(ev[index & ~1].astype(">u8").tobytes() + ev[index | 1].astype(">u8").tobytes())
            assert R.fold_path(leaf, index >> 1, gp) == layers[k][2]


def test_open_deep_composition_poly(tree_cases):
    import torch
    from lambda_elliptic_curves_amd import fft, merkle, stark
    F, name, log2_rows = fft.Stark252PrimeField, "stark252", 5
    rows = 1 << log2_rows
    rng = np.random.default_rng(3)
    srcs, hosts = {}, {}
    for key, n_cols, seed in (("main", 3, 1), ("aux", 2, 2), ("composition", 2, 3)):
        host = util.rand_elems(name, n_cols * rows, 8100 + seed).reshape(n_cols, rows, 4)
        t_cols = cuda(host)
        if key == "composition":
            nodes = rng.integers(0, 256, (rows - 1, 32), dtype=np.uint8)
            t_nodes = cuda(nodes.view(np.uint64))
        else:
            t_nodes = torch.empty((2 * rows - 1) * 4, dtype=torch.int64, device="cuda")
            merkle.commit_columns_device(F, t_cols, n_cols, log2_rows, t_nodes)
            nodes = t_nodes.cpu().numpy().view(np.uint8).reshape(-1, 32)
        srcs[key], hosts[key] = (t_cols, n_cols, log2_rows, t_nodes), (host, nodes)
    iotas = [0, rows // 2 - 1, 5, 5]
    for aux in (None, srcs["aux"]):
        got = stark.open_deep_composition_poly_device(F, srcs["main"], srcs["composition"], iotas, aux=aux)
        assert len(got) == len(iotas)
        for entry, iota in zip(got, iotas):
            assert set(entry) == {"main", "composition"} | ({"aux"} if aux is not None else set())
            for key in entry:
                host, nodes = hosts[key]
                want = (R.open_composition_poly if key == "composition" else R.open_trace_polys)(host, nodes, log2_rows, iota)
                for field in ("evaluations", "evaluations_sym", "proof", "proof_sym"):
                    assert entry[key][field].shape == want[field].shape and np.array_equal(entry[key][field], want[field]), (key, field)


def test_stone_compat_auth_path_from_the_device_tree(kats):
    import torch
    from lambda_elliptic_curves_amd import fft, merkle
    case, cols, pos = stone_case_1_opening(kats)
    F, log2_rows = fft.Stark252PrimeField, cols.shape[1].bit_length() - 1
    t_cols = cuda(cols)
    t_nodes = torch.empty((2 * cols.shape[1] - 1) * 4, dtype=torch.int64, device="cuda")
    root = merkle.commit_columns_device(F, t_cols, 2, log2_rows, t_nodes)
    assert root.hex() == case["root"]
    tree = merkle.Tree(F, t_nodes, log2_rows, t_columns=t_cols, n_cols=2)
    values, paths = merkle.open_trees_device([tree], [[pos, pos + 1]])
    assert [bytes(x).hex() for x in paths[0][0][1:4]] == case["auth_path_nodes"]
    assert np.array_equal(values[0][0, 0], cols[:, R.bitrev(pos, log2_rows)])
    assert np.array_equal(values[0][1, 0], cols[:, R.bitrev(pos + 1, log2_rows)])
