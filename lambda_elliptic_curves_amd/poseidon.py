"""Host-side mirror of the reference's Starknet Poseidon (crypto/src/hash/poseidon/mod.rs, PoseidonCairoStark252) and of
the Merkle trees built on it (TreePoseidon, BatchPoseidonTree), batched on the device.  Elements are Stark252
FieldElements as everywhere else: (…, 4) uint64, most significant limb first, Montgomery form, canonical."""
import numpy as np

from . import _lib as L, _tree
from ._lib import device_ptr as _dp, host_ptr as _vp, stream_ptr as _stream
from .errors import check

LEAF_SINGLE, LEAF_MANY = L.POSEIDON_LEAF_SINGLE, L.POSEIDON_LEAF_MANY


def _elems(a, shape):
    return np.ascontiguousarray(a, dtype=np.uint64).reshape(shape)


def permute(states):
    """hades_permutation of every state: (n, 3, 4) -> (n, 3, 4)"""
    s = _elems(states, (-1, 3, 4))
    out = np.zeros_like(s)
    check(L.lib().lw_poseidon_permute(_vp(s), s.shape[0], _vp(out)))
    return out


def hash(x, y):
    """hash(x[i], y[i]): (n, 4), (n, 4) -> (n, 4)"""
    x, y = _elems(x, (-1, 4)), _elems(y, (-1, 4))
    if x.shape != y.shape:
        raise ValueError("hash: one y per x")
    out = np.zeros_like(x)
    check(L.lib().lw_poseidon_hash(_vp(x), _vp(y), x.shape[0], _vp(out)))
    return out


def hash_single(x):
    """hash_single(x[i]): (n, 4) -> (n, 4)"""
    x = _elems(x, (-1, 4))
    out = np.zeros_like(x)
    check(L.lib().lw_poseidon_hash_single(_vp(x), x.shape[0], _vp(out)))
    return out


def hash_many(rows):
    """hash_many of every row: (n_rows, row_len, 4) -> (n_rows, 4); row_len = 0 hashes the padding block alone"""
    r = np.ascontiguousarray(rows, dtype=np.uint64)
    if r.ndim != 3 or r.shape[2] != 4:
        raise ValueError("hash_many: rows is (n_rows, row_len, 4)")
    out = np.zeros((r.shape[0], 4), np.uint64)
    check(L.lib().lw_poseidon_hash_many(_vp(r), r.shape[0], r.shape[1], _vp(out)))
    return out


def commit_columns(columns, leaf_mode=LEAF_MANY, bit_reverse=True, return_nodes=False):
    """columns: (n_cols, N, 4) natural-order columns.  leaf_mode LEAF_SINGLE: TreePoseidon (one column, leaf =
    hash_single); LEAF_MANY: BatchPoseidonTree (leaf = hash_many of the row).  Returns the root element (4,) uint64 (and
    the reference's `nodes`, (2N - 1, 4) root first, when return_nodes)."""
    cols = np.ascontiguousarray(columns, dtype=np.uint64)
    return _tree.commit_host(cols, 4, np.uint64, return_nodes, lambda log2n, root, nodes: L.lib().lw_poseidon_commit_columns(
        _vp(cols), cols.shape[0], log2n, 1 if bit_reverse else 0, leaf_mode, root, nodes))


# ---- device-resident forms: torch int64 tensors holding the same (…, 4) limbs, 16-byte aligned
def permute_device(t_states, n, t_out=None, stream=None):
    """n states of 3 elements in t_states -> t_out (default: in place)"""
    t_out = t_states if t_out is None else t_out
    check(L.lib().lw_poseidon_permute_device(_dp(t_states), n, _dp(t_out), _stream(stream)))
    return t_out


def hash_device(t_x, t_y, n, t_out, stream=None):
    check(L.lib().lw_poseidon_hash_device(_dp(t_x), _dp(t_y), n, _dp(t_out), _stream(stream)))
    return t_out


def hash_single_device(t_x, n, t_out, stream=None):
    check(L.lib().lw_poseidon_hash_single_device(_dp(t_x), n, _dp(t_out), _stream(stream)))
    return t_out


def hash_many_device(t_rows, n_rows, row_len, t_out, stream=None):
    check(L.lib().lw_poseidon_hash_many_device(_dp(t_rows) if row_len else None, n_rows, row_len, _dp(t_out), _stream(stream)))
    return t_out


def commit_columns_device(t_columns, n_cols, log2n, t_nodes, leaf_mode=LEAF_MANY, bit_reverse=True, col_stride_elems=0,
                          return_root=True, stream=None):
    """t_columns: n_cols columns of 2^log2n elements, col_stride_elems apart (0: dense); t_nodes: (2 * 2^log2n - 1) x 4
    int64, the reference's `nodes` (readable by merkle.open_trees_device as it is).  Returns the root element (4,) uint64
    after synchronising the stream, or None (nothing waited for) with return_root=False."""
    return _tree.commit_device(4, np.uint64, return_root, lambda root: L.lib().lw_poseidon_commit_columns_device(
        _dp(t_columns), n_cols, col_stride_elems, log2n, 1 if bit_reverse else 0, leaf_mode, _dp(t_nodes), root, _stream(stream)))
