"""Host-side mirror of the reference's Monolith over Mersenne31 (crypto/src/hash/monolith/, MonolithMersenne31<WIDTH,
NUM_FULL_ROUNDS>, ported there from Plonky3), batched on the device, and of the hash, the 2-to-1 compression and the
Merkle tree that Plonky3 builds from the width-16 permutation.

A word is one uint32, as in circle.py: any word is accepted and read mod p = 2^31 - 1, every word of a result is the
canonical residue.  `width` is 8, 12, 16, 20 or 24, `rounds` (NUM_FULL_ROUNDS) 1 .. 15; the reference tests 5.  Host arrays
are numpy uint32; the device entry points take torch int32 tensors of the same bytes, 16-byte aligned, and run on torch's
current stream.
"""
import numpy as np

from . import _lib as L, _tree
from ._lib import device_ptr as _dp, host_ptr as _vp, stream_ptr as _stream
from .errors import check

P = (1 << 31) - 1
WIDTHS = (8, 12, 16, 20, 24)
MAX_ROUNDS = 15
DIGEST_LEN, RATE, SPONGE_WIDTH = 8, 8, 16
LAYER_CONCRETE, LAYER_BARS, LAYER_BRICKS = L.MONOLITH_CONCRETE, L.MONOLITH_BARS, L.MONOLITH_BRICKS


def _instance(width, rounds):
    if width not in WIDTHS:
        raise ValueError(f"monolith: width is one of {WIDTHS}, not {width!r}")
    _rounds(rounds)


def _rounds(rounds):
    if not isinstance(rounds, int) or not 1 <= rounds <= MAX_ROUNDS:
        raise ValueError(f"monolith: rounds is 1 .. {MAX_ROUNDS}, not {rounds!r}")


def constants(width, rounds):
    """-> (round constants (rounds, width), the matrix of Concrete (width, width)) of one instance, generated from their
    SHAKE128 rule; for width 16 the matrix is the circulant written out.  Needs no device."""
    _instance(width, rounds)
    rc, mds = np.zeros((rounds, width), np.uint32), np.zeros((width, width), np.uint32)
    check(L.lib().lw_monolith_constants(width, rounds, _vp(rc), _vp(mds)))
    return rc, mds


def permute(width, rounds, states):
    """permutation() of every state: (n, width) -> (n, width)"""
    _instance(width, rounds)
    s = np.ascontiguousarray(states, dtype=np.uint32).reshape(-1, width)
    out = np.zeros_like(s)
    check(L.lib().lw_monolith_permute(width, rounds, _vp(s), s.shape[0], _vp(out)))
    return out


def hash(rounds, rows):
    """The digest of every row: (n_rows, row_len) -> (n_rows, 8); a single sequence (row_len,) -> (8,).  The state starts
    as 16 zeros, every chunk of up to 8 words overwrites its front and the state is permuted; row_len = 0 gives zeros.
    There is no padding, so the hash is only meant for rows of one fixed length: [a] and [a, 0] have the same digest."""
    _rounds(rounds)
    r = np.ascontiguousarray(rows, dtype=np.uint32)
    single = r.ndim == 1
    if single:
        r = r.reshape(1, -1)
    if r.ndim != 2:
        raise ValueError("hash: rows is (n_rows, row_len)")
    out = np.zeros((r.shape[0], DIGEST_LEN), np.uint32)
    check(L.lib().lw_monolith_hash(rounds, _vp(r), r.shape[0], r.shape[1], _vp(out)))
    return out[0] if single else out


def compress(rounds, left, right):
    """permute(left[i] || right[i])[0:8], the parent of two digests: (n, 8), (n, 8) -> (n, 8)"""
    _rounds(rounds)
    a = np.ascontiguousarray(left, dtype=np.uint32).reshape(-1, DIGEST_LEN)
    b = np.ascontiguousarray(right, dtype=np.uint32).reshape(-1, DIGEST_LEN)
    if a.shape != b.shape:
        raise ValueError("compress: one right digest per left digest")
    out = np.zeros_like(a)
    check(L.lib().lw_monolith_compress(rounds, _vp(a), _vp(b), a.shape[0], _vp(out)))
    return out


def commit_columns(rounds, columns, bit_reverse=True, return_nodes=False):
    """columns: (n_cols, N) natural-order columns of words.  Leaf j = hash of committed row j (natural row bitrev(j) with
    bit_reverse), node = compress.  Returns the root (8,) uint32 (and `nodes`, (2N - 1, 8) root first in the layout of
    the reference's trees, when return_nodes)."""
    _rounds(rounds)
    cols = np.ascontiguousarray(columns, dtype=np.uint32)
    if cols.ndim != 2 or cols.shape[0] == 0:
        raise ValueError("commit_columns: columns is (n_cols, N) with at least one column")
    return _tree.commit_host(cols, DIGEST_LEN, np.uint32, return_nodes, lambda log2n, root, nodes: L.lib().lw_monolith_commit_columns(
        rounds, _vp(cols), cols.shape[0], log2n, 1 if bit_reverse else 0, root, nodes))


# ---- device-resident forms: torch int32 tensors holding the same words, 16-byte aligned
def permute_device(width, rounds, t_states, n, t_out=None, stream=None):
    """n states in t_states -> t_out (default: in place)"""
    t_out = t_states if t_out is None else t_out
    check(L.lib().lw_monolith_permute_device(width, rounds, _dp(t_states), n, _dp(t_out), _stream(stream)))
    return t_out


def layer_device(width, rounds, layer, t_states, n, t_out=None, stream=None):
    """Test seam: one layer (LAYER_CONCRETE, LAYER_BARS, LAYER_BRICKS) of every state, through the function the
    permutation inlines -> t_out (default: in place)"""
    t_out = t_states if t_out is None else t_out
    check(L.lib().lw_monolith_layer_device(width, rounds, layer, _dp(t_states), n, _dp(t_out), _stream(stream)))
    return t_out


def hash_device(rounds, t_rows, n_rows, row_len, t_out, row_stride=0, stream=None):
    """n_rows rows of row_len words, row_stride words apart (0: dense) -> n_rows digests in t_out"""
    check(L.lib().lw_monolith_hash_device(rounds, _dp(t_rows) if row_len else None, n_rows, row_len, row_stride, _dp(t_out), _stream(stream)))
    return t_out


def compress_device(rounds, t_left, t_right, n, t_out, stream=None):
    """n left and n right digests -> their n parents in t_out"""
    check(L.lib().lw_monolith_compress_device(rounds, _dp(t_left), _dp(t_right), n, _dp(t_out), _stream(stream)))
    return t_out


def commit_columns_device(rounds, t_columns, n_cols, log2n, t_nodes, bit_reverse=True, col_stride=0, return_root=True, stream=None):
    """t_columns: n_cols columns of 2^log2n words, col_stride words apart (0: dense), e.g. the output of circle.lde_device
    as it lies; t_nodes: (2 * 2^log2n - 1) x 8 int32, the tree (readable by merkle.open_trees_device as it is).  Returns
    the root (8,) uint32 after synchronising the stream, or None (nothing waited for) with return_root=False."""
    return _tree.commit_device(DIGEST_LEN, np.uint32, return_root, lambda root: L.lib().lw_monolith_commit_columns_device(
        rounds, _dp(t_columns), n_cols, col_stride, log2n, 1 if bit_reverse else 0, _dp(t_nodes), root, _stream(stream)))
