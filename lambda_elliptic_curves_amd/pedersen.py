"""Host-side mirror of the reference's Starknet Pedersen hash (crypto/src/hash/pedersen/mod.rs, PedersenStarkCurve::hash)
and of the 2-to-1 Merkle tree over leaf values built on it (the reference's MerkleTree with hash_new_parent = the hash and
identity leaves), batched on the device.  Elements are Stark252 FieldElements as everywhere else: (…, 4) uint64, most
significant limb first, Montgomery form, canonical.  Points are affine (x, y): (…, 2, 4)."""
import numpy as np

from . import _lib as L, _tree
from ._lib import device_ptr as _dp, host_ptr as _vp, stream_ptr as _stream
from .errors import check

N_POINTS = 1890   # T1 || T2 || T3 || T4: 930 + 15 + 930 + 15


def _elems(a, shape):
    return np.ascontiguousarray(a, dtype=np.uint64).reshape(shape)


def hash(x, y):
    """hash(x[i], y[i]): (n, 4), (n, 4) -> (n, 4)"""
    x, y = _elems(x, (-1, 4)), _elems(y, (-1, 4))
    if x.shape != y.shape:
        raise ValueError("hash: one y per x")
    out = np.zeros_like(x)
    check(L.lib().lw_pedersen_hash(_vp(x), _vp(y), x.shape[0], _vp(out)))
    return out


def commit_leaves(leaves, bit_reverse=True, return_nodes=False):
    """leaves: (N, 4) leaf values in natural order, or (n_cols, N, 4) with n_cols = 1 (anything else is refused by the
    library).  Returns the root element (4,) uint64 (and the reference's `nodes`, (2N - 1, 4) root first, leaves last, when
    return_nodes)."""
    cols = np.ascontiguousarray(leaves, dtype=np.uint64)
    if cols.ndim == 2:
        cols = cols.reshape(1, -1, 4)
    return _tree.commit_host(cols, 4, np.uint64, return_nodes, lambda log2n, root, nodes: L.lib().lw_pedersen_commit_leaves(
        _vp(cols), cols.shape[0], log2n, 1 if bit_reverse else 0, root, nodes))


def table():
    """the 1 890 affine points of the lookup tables, generated from the five published points: (1890, 2, 4); no device needed"""
    out = np.zeros((N_POINTS, 2, 4), np.uint64)
    check(L.lib().lw_pedersen_table(_vp(out)))
    return out


# ---- device-resident forms: torch int64 tensors holding the same (…, 4) limbs, 16-byte aligned
def hash_device(t_x, t_y, n, t_out, stream=None):
    check(L.lib().lw_pedersen_hash_device(_dp(t_x), _dp(t_y), n, _dp(t_out), _stream(stream)))
    return t_out


def commit_leaves_device(t_leaves, log2n, t_nodes, bit_reverse=True, return_root=True, n_cols=1, stream=None):
    """t_leaves: 2^log2n leaf values; t_nodes: (2 * 2^log2n - 1) x 4 int64, the reference's `nodes` (readable by
    merkle.open_trees_device as it is).  Returns the root element (4,) uint64 after synchronising the stream, or None
    (nothing waited for) with return_root=False."""
    return _tree.commit_device(4, np.uint64, return_root, lambda root: L.lib().lw_pedersen_commit_leaves_device(
        _dp(t_leaves), n_cols, log2n, 1 if bit_reverse else 0, _dp(t_nodes), root, _stream(stream)))


def add_affine_device(t_p, t_z, t_q, n, t_out, stream=None):
    """test seam of the group law: t_out[i] = t_p[i] + t_q[i], affine points of (2, 4) limbs, (0, 0) the point at infinity in
    t_p and t_out; t_p[i] goes through the hash kernel's accumulator representation rescaled by the element t_z[i] != 0"""
    check(L.lib().lw_pedersen_add_affine_device(_dp(t_p), _dp(t_z), _dp(t_q), n, _dp(t_out), _stream(stream)))
    return t_out
