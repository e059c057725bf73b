"""The Keccak-256 commitment (csrc/merkle.hip) and the FRI layer (csrc/fri.hip) where test_gpu_merkle.py does not reach:
strided columns between canaries, Fr381, every sponge seam of the three element widths, every level schedule, and the
fold at operands where its additions cross the modulus, into buffers that were dirty before.  Every comparison is byte
equality."""
import hashlib

import numpy as np
import pytest

from oracle import bigint_def as D
from oracle import oracle as O
from tests import keccak_tree_ref as K
from tests import util

pytestmark = pytest.mark.gpu

FIELDS = {"stark252": (O.F_STARK252, D.P_STARK252), "fr381": (O.F_FR381, D.P_FR381)}
CANARY64 = 0xDEADBEEFCAFEF00D
CANARY32 = 0xDEADBEEF
CANARY_I64 = CANARY64 - (1 << 64)   # the same word as torch sees it
GUARD = 4   # digests behind the node array


def _columns(name, n_cols, n, seed):
    cols = np.stack([util.rand_elems(name, n, seed + 13 * c) for c in range(n_cols)])
    assert len({cols[c].tobytes() for c in range(n_cols)}) == n_cols   # a column read twice cannot stand in for another
    return cols


def _oracle_tree(cols, bit_reverse):
    threads = util.host_threads() if cols.shape[1] > (1 << 14) else 1
    if cols.ndim == 3:
        return O.merkle_commit_columns(cols, bit_reverse, threads=threads)
    return O.merkle_commit_columns_babybear(cols, bit_reverse, threads=threads)


def _signed(a):
    return np.ascontiguousarray(a).view(np.int32 if a.dtype == np.uint32 else np.int64)


def _to_device(a):
    import torch
    return torch.from_numpy(_signed(a).copy()).cuda()


def _commit(name, t_cols, n_cols, log2n, t_nodes, **kw):
    """the 256-bit fields through lw_stark_commit_columns_device, BabyBear through the layout entry"""
    from lambda_elliptic_curves_amd import merkle
    entry = merkle.commit_columns_device if name in FIELDS else merkle.commit_columns_layout_device
    return entry(util.fld(name), t_cols, n_cols, log2n, t_nodes, **kw)


def _node_buffer(n):
    """(2n - 1 + GUARD) digests, every word a canary"""
    import torch
    return torch.full(((2 * n - 1 + GUARD) * 4,), CANARY_I64, dtype=torch.int64, device="cuda")


def _nodes_and_guard(t_nodes, n):
    got = t_nodes.cpu().numpy().view(np.uint8).reshape(2 * n - 1 + GUARD, 32)
    return got[:2 * n - 1], got[2 * n - 1:]


def _guard_intact(guard):
    return guard.tobytes() == np.full(guard.size // 8, CANARY64, np.uint64).tobytes()


# ---- 1. the column stride
_STRIDED = {}


def _strided_case(name, n_cols, log2n):
    """columns and both oracle trees, computed once per (layout, shape) and shared by the two paddings"""
    key = (name, n_cols, log2n)
    if key not in _STRIDED:
        cols = _columns(name, n_cols, 1 << log2n, 2300 + 7 * log2n)
        trees = {br: _oracle_tree(cols, br) for br in (True, False)}
        for a in (cols, *trees.values()):
            a.setflags(write=False)
        _STRIDED[key] = (cols, trees)
    return _STRIDED[key]


def _check_strided(name, n_cols, log2n, pad, use_stream=False):
    import torch
    n = 1 << log2n
    stride = n + pad
    cols, trees = _strided_case(name, n_cols, log2n)
    canary = cols.dtype.type(CANARY32 if cols.dtype == np.uint32 else CANARY64)
    buf = np.full((n_cols, stride) + cols.shape[2:], canary, cols.dtype)   # the gap behind the last column too
    buf[:, :n] = cols
    t_buf, t_dense = _to_device(buf), _to_device(cols)
    kw = {}
    if use_stream:
        side = torch.cuda.Stream()
        torch.cuda.synchronize()   # the uploads and fills below run on the default stream
        kw["stream"] = side.cuda_stream
    for br in (True, False):
        t_nodes, t_nodes_dense = _node_buffer(n), _node_buffer(n)
        torch.cuda.synchronize()
        root = _commit(name, t_buf, n_cols, log2n, t_nodes, bit_reverse=br, col_stride_elems=stride, **kw)
        root_dense = _commit(name, t_dense, n_cols, log2n, t_nodes_dense, bit_reverse=br, col_stride_elems=0, **kw)
        if use_stream:
            side.synchronize()
        nodes, guard = _nodes_and_guard(t_nodes, n)
        assert nodes.tobytes() == trees[br].tobytes(), (br, "nodes")
        assert root == nodes[0].tobytes() == root_dense
        assert _guard_intact(guard), (br, "guard digests")
        dense_nodes, dense_guard = _nodes_and_guard(t_nodes_dense, n)
        assert dense_nodes.tobytes() == nodes.tobytes() and _guard_intact(dense_guard), (br, "dense")
        assert t_buf.cpu().numpy().tobytes() == buf.tobytes(), (br, "input buffer")


# the top kernel alone (2^0, 2^3, 2^9), 1 and 4 levels fused into the leaf kernel (2^10, 2^13), 4 fused levels and a launch of
# 2 more behind them (2^15), and 2^17: the tiled bit-reversed gather, then a launch of 1, of 4 and of 3 levels
@pytest.mark.parametrize("pad", [1, 24])   # 1: 4-byte columns start off 8-byte alignment
@pytest.mark.parametrize("n_cols,log2n", [(1, 0), (3, 3), (2, 9), (5, 10), (3, 13), (2, 15), (2, 17)])
@pytest.mark.parametrize("name", ["stark252", "fr381", "babybear_u64", "babybear_u32"])
def test_strided_columns_between_canaries(name, n_cols, log2n, pad):
    _check_strided(name, n_cols, log2n, pad)


@pytest.mark.parametrize("name", ["stark252", "babybear_u32"])
def test_strided_columns_on_a_side_stream(name):
    _check_strided(name, 5, 10, 1, use_stream=True)


def test_stride_below_the_column_length_is_refused():
    from lambda_elliptic_curves_amd import errors, poseidon
    n_cols, log2n = 2, 3
    for name in ("stark252", "babybear_u32"):
        t_cols = _to_device(_columns(name, n_cols, 1 << log2n, 40))
        t_nodes = _node_buffer(1 << log2n)
        with pytest.raises(errors.HipError, match="below the column length"):
            _commit(name, t_cols, n_cols, log2n, t_nodes, col_stride_elems=7)
        nodes, guard = _nodes_and_guard(t_nodes, 1 << log2n)
        assert _guard_intact(nodes) and _guard_intact(guard)   # nothing ran
    t_cols = _to_device(_columns("stark252", n_cols, 1 << log2n, 41))
    with pytest.raises(errors.HipError, match="below the column length"):
        poseidon.commit_columns_device(t_cols, n_cols, log2n, _node_buffer(1 << log2n), col_stride_elems=7)


# ---- 2. sponge seams: the leaf's bytes end just before, at and just behind a block of the rate, for each element width
SEAMS = ([("stark252", c) for c in K.SEAM_COLS[32]] + [("fr381", 4), ("fr381", 17)] +
         [("babybear_u64", c) for c in K.SEAM_COLS[8]] + [("babybear_u32", c) for c in K.SEAM_COLS[4]])


@pytest.mark.parametrize("name,n_cols", SEAMS)
def test_sponge_seams_match_the_plain_tree(name, n_cols):
    log2n, n = 3, 8
    cols = _columns(name, n_cols, n, 3100 + n_cols)
    t_cols = _to_device(cols)
    for br in (True, False):
        exp = K.keccak_tree(cols, br)
        t_nodes = _node_buffer(n)
        root = _commit(name, t_cols, n_cols, log2n, t_nodes, bit_reverse=br)
        nodes, guard = _nodes_and_guard(t_nodes, n)
        assert nodes.tobytes() == exp.tobytes(), br
        assert root == exp[0].tobytes() and _guard_intact(guard)


# ---- 3. every level schedule: the top kernel alone up to 2^9, 1 - 4 levels fused into the leaf kernel from 2^10 to 2^13, 4
# fused and a launch of 1 - 3 levels behind them from 2^14 to 2^16, above that no fused leaf levels, the tiled gather and a
# launch per level down to 2^16
@pytest.mark.parametrize("log2n", range(19))
@pytest.mark.parametrize("name,n_cols", [("stark252", 1), ("babybear_u32", 3)])
def test_every_level_schedule(name, n_cols, log2n):
    n = 1 << log2n
    cols = _columns(name, n_cols, n, 5200 + log2n)
    exp = _oracle_tree(cols, True)
    t_nodes = _node_buffer(n)
    root = _commit(name, _to_device(cols), n_cols, log2n, t_nodes, bit_reverse=True)
    nodes, guard = _nodes_and_guard(t_nodes, n)
    assert nodes.tobytes() == exp.tobytes()
    assert root == exp[0].tobytes() and _guard_intact(guard)


# ---- 4. Fr381 through a whole commit phase
def _layer_oracle(f, poly, domain, off):
    """new_fri_layer of the (stripped) polynomial: bit-reversed evaluation and the tree over its pairs"""
    ev = O.bit_reverse_permute(f, O.evaluate_fft(f, poly, 1, domain, off)) if len(poly) else np.zeros((domain, 4), np.uint64)
    leaves = ev.reshape(domain // 2, 2, 4)
    return ev, O.merkle_commit_columns(np.ascontiguousarray(leaves.transpose(1, 0, 2)), bit_reverse=False)


def test_fr381_commit_phase_every_layer():
    """commit_phase (provers/stark/src/fri/mod.rs:22-75) over Fr381: 2^6 coefficients, blow-up 4, down to the constant, under
    a hash-chain transcript; every layer's evaluation, node array and root, and the last value."""
    from lambda_elliptic_curves_amd import merkle
    f, p = FIELDS["fr381"]
    log_coeffs, h = 6, 3
    n, domain = 1 << log_coeffs, 4 << log_coeffs
    a = util.rand_elems("fr381", n, 9300)
    a[-1, -1] |= np.uint64(1)
    state = {"s": b"fri-fr381", "zetas": []}

    def sample_zeta():
        z = int.from_bytes(hashlib.sha256(state["s"]).digest()[:31], "big")   # canonical, below 2^248
        state["zetas"].append(z)
        state["s"] = hashlib.sha256(state["s"] + b"z").digest()
        return O.elems_to_mont(f, [z])[0]

    def append_root(root):
        state["s"] = hashlib.sha256(state["s"] + root).digest()

    offset_sq = lambda k: O.elems_to_mont(f, [pow(h, 1 << k, p)])[0]
    t_last, layers = merkle.fri_commit_phase_device(util.fld("fr381"), log_coeffs + 1, util.dev(a), n, sample_zeta, append_root,
                                                    offset_sq, domain)
    assert len(layers) == log_coeffs and len(set(state["zetas"])) == log_coeffs + 1
    poly, dom = a, domain
    for k, (t_ev, t_nodes, root, dsize) in enumerate(layers, start=1):
        poly = O.fri_fold_twice(f, poly, O.elems_to_mont(f, [state["zetas"][k - 1]])[0])
        dom //= 2
        assert dsize == dom
        ev, exp_nodes = _layer_oracle(f, poly, dom, offset_sq(k))
        assert util.host(t_ev).tobytes() == ev.tobytes(), f"layer {k} evaluation"
        assert t_nodes.cpu().numpy().view(np.uint8).tobytes() == exp_nodes.tobytes(), f"layer {k} tree"
        assert root == exp_nodes[0].tobytes(), f"layer {k} root"
    last = O.fri_fold_twice(f, poly, O.elems_to_mont(f, [state["zetas"][-1]])[0], strip=False)
    assert last.shape[0] == 1
    assert util.host(t_last)[0].tobytes() == last[0].tobytes()


# ---- 5. the fold: dirty buffers, guard elements, operands at the edges
def _strip(vals):
    vals = list(vals)
    while vals and vals[-1] == 0:
        vals.pop()
    return vals


def _layer_buffers(blk, domain):
    """the caller's buffers of fri_layer_device, every word a canary: the block and the evaluation 2 elements longer than
    asked for, the nodes GUARD digests longer"""
    import torch
    c = CANARY_I64
    return (torch.full((blk + 2, 4), c, dtype=torch.int64, device="cuda"),
            torch.full((domain + 2, 4), c, dtype=torch.int64, device="cuda"),
            torch.full(((domain - 1 + GUARD) * 4,), c, dtype=torch.int64, device="cuda"))


def _check_layer(name, stored, zeta, domain, bufs=None):
    """fri_layer_device on the coefficients `stored` (integers, stored form) into canary-filled (or the given) buffers
    against Python integers for the fold and the oracle for the layer; returns the buffers and their contents"""
    from lambda_elliptic_curves_amd import merkle
    f, p = FIELDS[name]
    n = len(stored)
    n_out = (n + 1) // 2
    blk = max(2, 1 << (n_out - 1).bit_length())
    off = O.elems_to_mont(f, [9])[0]
    exp = K.fold_twice_stored(p, stored, zeta)
    assert len(exp) == n_out and all(v < p for v in exp)
    bufs = bufs or _layer_buffers(blk, domain)
    t_in = util.dev(util.to_arr(stored))
    t_poly, got_n_out, t_ev, t_nodes, root = merkle.fri_layer_device(util.fld(name), t_in, n, util.to_arr([zeta]), off, domain, buffers=bufs)
    assert got_n_out == n_out and t_poly is bufs[0]
    poly = util.to_ints(util.host(t_poly))
    assert len(poly) == blk + 2
    assert poly[:n_out] == exp, "fold"
    assert all(v < p for v in poly[:n_out]), "canonical residues"
    assert poly[n_out:blk] == [0] * (blk - n_out), "zero padding of the block"
    canary_elem = int.from_bytes(CANARY64.to_bytes(8, "big") * 4, "big")
    assert poly[blk:] == [canary_elem] * 2, "guard elements of the block"
    # the NTT reads the whole block: with anything but zeros behind n_out the evaluation could not be the oracle's
    ev, exp_nodes = _layer_oracle(f, util.to_arr(_strip(exp)), domain, off)
    got_ev = util.host(t_ev)
    assert got_ev[:domain].tobytes() == ev.tobytes(), "evaluation"
    assert util.to_ints(got_ev[domain:]) == [canary_elem] * 2, "guard elements of the evaluation"
    got_nodes = t_nodes.cpu().numpy().view(np.uint8).reshape(domain - 1 + GUARD, 32)
    assert got_nodes[:domain - 1].tobytes() == exp_nodes.tobytes(), "tree"
    assert root == exp_nodes[0].tobytes() and _guard_intact(got_nodes[domain - 1:])
    assert util.host(t_in).tobytes() == util.to_arr(stored).tobytes(), "input"
    return bufs, (util.host(t_poly).tobytes(), got_ev.tobytes(), got_nodes.tobytes(), root)


def _check_fold(name, stored, zeta):
    """fri_fold_device alone; it allocates its block itself, so a block of the same size full of canaries is handed back to
    the allocator just before"""
    import torch
    from lambda_elliptic_curves_amd import merkle
    p = FIELDS[name][1]
    n = len(stored)
    n_out = (n + 1) // 2
    blk = max(2, 1 << (n_out - 1).bit_length())
    exp = K.fold_twice_stored(p, stored, zeta)
    t_in = util.dev(util.to_arr(stored))
    dirty = torch.full((blk, 4), CANARY_I64, dtype=torch.int64, device="cuda")
    del dirty
    t_poly, got_n_out = merkle.fri_fold_device(util.fld(name), t_in, n, util.to_arr([zeta]))
    poly = util.to_ints(util.host(t_poly))
    assert got_n_out == n_out and len(poly) == blk
    assert poly[:n_out] == exp, "fold"
    assert poly[n_out:] == [0] * (blk - n_out), "zero padding of the block"
    assert util.host(t_in).tobytes() == util.to_arr(stored).tobytes(), "input"


@pytest.mark.parametrize("reading", ["stored", "canonical"])
@pytest.mark.parametrize("name", ["stark252", "fr381"])
def test_fold_at_the_edges(name, reading):
    """Every ordered pair of {0, 1, 2, p-1, p-2, (p-1)/2, (p+1)/2} and one unpaired p-1, under each of these as zeta and
    one random zeta.  `stored`: the words in memory are these numbers, so c0 + zeta*c1 and the doubling add residues that
    sit at the modulus; `canonical`: the elements stand for these numbers (zeta = 0, 1, -1 among them)."""
    p = FIELDS[name][1]
    to_stored = (lambda v: v) if reading == "stored" else (lambda v: v * K.R256 % p)
    coeffs = [to_stored(v) for v in K.edge_coeffs(p)]
    zetas = [to_stored(z) for z in K.edge_values(p)] + [util.to_ints(util.rand_elems(name, 1, 77))[0]]
    for z in zetas:
        _check_fold(name, coeffs, z)
        _check_layer(name, coeffs, z, 64)


# the unpaired tail on each side of the 256-work-item boundary; 513, 514: a block of 512 that is mostly padding
@pytest.mark.parametrize("n_coeffs", [1, 2, 3, 511, 512, 513, 514])
@pytest.mark.parametrize("name", ["stark252", "fr381"])
def test_fold_lengths_into_dirty_buffers(name, n_coeffs):
    stored = util.to_ints(util.rand_elems(name, n_coeffs, 6100 + n_coeffs))
    stored[-1] |= 1
    zeta = util.to_ints(util.rand_elems(name, 1, 6200 + n_coeffs))[0]
    n_out = (n_coeffs + 1) // 2
    blk = max(2, 1 << (n_out - 1).bit_length())
    assert blk == {1: 2, 2: 2, 3: 2, 511: 256, 512: 256, 513: 512, 514: 512}[n_coeffs]
    _check_fold(name, stored, zeta)
    _check_layer(name, stored, zeta, 2 * blk)


@pytest.mark.parametrize("name", ["stark252", "fr381"])
def test_fold_twice_into_the_same_dirty_buffers(name):
    stored = util.to_ints(util.rand_elems(name, 33, 6300))
    stored[-1] |= 1
    zeta = util.to_ints(util.rand_elems(name, 1, 6301))[0]
    bufs, first = _check_layer(name, stored, zeta, 64)
    # a longer polynomial in between leaves the whole block non-zero
    other = util.to_ints(util.rand_elems(name, 64, 6302))
    from lambda_elliptic_curves_amd import merkle
    merkle.fri_layer_device(util.fld(name), util.dev(util.to_arr(other)), 64, util.to_arr([zeta]), O.elems_to_mont(FIELDS[name][0], [9])[0], 64,
                            buffers=bufs)
    assert all(v != 0 for v in util.to_ints(util.host(bufs[0]))[:32])
    _, second = _check_layer(name, stored, zeta, 64, bufs=bufs)
    assert second == first
