"""Host-side mirror of the reference's Rescue Prime Optimized over Goldilocks (crypto/src/hash/rescue_prime/,
RescuePrimeOptimized; ePrint 2022/1577) and of a Merkle tree built from its `hash`, batched on the device.

A word is one uint64, the residue itself, as in goldilocks.py: any word is accepted and read mod p, every word of a result
is the canonical residue.  `level` is LEVEL_128 (state 12, rate 8, digest 4 words: the hash of Miden) or LEVEL_160 (state
16, rate 10, digest 5 words).  Host arrays are numpy uint64; the device entry points take torch int64 tensors of the same
bytes, 16-byte aligned, and run on torch's current stream.
"""
import numpy as np

from . import _lib as L, _tree
from ._lib import device_ptr as _dp, host_ptr as _vp, stream_ptr as _stream
from .errors import check

P = (1 << 64) - (1 << 32) + 1
LEVEL_128, LEVEL_160 = L.RPO_128, L.RPO_160
_SHAPE = {LEVEL_128: (12, 4, 8), LEVEL_160: (16, 6, 10)}   # level -> (state width, capacity, rate)


def _params(level):
    if level not in _SHAPE:
        raise ValueError(f"rpo: level is LEVEL_128 or LEVEL_160, not {level!r}")
    return _SHAPE[level]


def state_width(level):
    return _params(level)[0]


def rate(level):
    return _params(level)[2]


def digest_len(level):
    return _params(level)[2] // 2


def permute(level, states):
    """permutation() of every state: (n, m) -> (n, m)"""
    m = state_width(level)
    s = np.ascontiguousarray(states, dtype=np.uint64).reshape(-1, m)
    out = np.zeros_like(s)
    check(L.lib().lw_rpo_permute(level, _vp(s), s.shape[0], _vp(out)))
    return out


def hash(level, rows):
    """hash() of every row: (n_rows, row_len) -> (n_rows, digest_len); a single sequence (row_len,) -> (digest_len,).
    row_len = 0 gives zeros, as the reference does."""
    _params(level)
    r = np.ascontiguousarray(rows, dtype=np.uint64)
    single = r.ndim == 1
    if single:
        r = r.reshape(1, -1)
    if r.ndim != 2:
        raise ValueError("hash: rows is (n_rows, row_len)")
    out = np.zeros((r.shape[0], digest_len(level)), np.uint64)
    check(L.lib().lw_rpo_hash(level, _vp(r), r.shape[0], r.shape[1], _vp(out)))
    return out[0] if single else out


def bytes_to_field_elements(data):
    """utils.rs:8-21: 7-byte little-endian chunks, a 1 byte appended to a short last chunk"""
    data = bytes(data)
    out = np.zeros((len(data) + 6) // 7, np.uint64)
    for k in range(out.shape[0]):
        chunk = data[7 * k:7 * k + 7]
        if len(chunk) < 7:
            chunk += b"\x01"
        out[k] = int.from_bytes(chunk, "little")
    return out


def hash_bytes(level, data):
    """hash_bytes(): bytes_to_field_elements on the host, then hash -> (digest_len,)"""
    return hash(level, bytes_to_field_elements(data))


def merge(level, left, right):
    """hash(left[i] || right[i]), the parent of two digests: (n, digest_len), (n, digest_len) -> (n, digest_len).  For
    LEVEL_128 this is Miden's 2-to-1 merge."""
    d = digest_len(level)
    a = np.ascontiguousarray(left, dtype=np.uint64).reshape(-1, d)
    b = np.ascontiguousarray(right, dtype=np.uint64).reshape(-1, d)
    if a.shape != b.shape:
        raise ValueError("merge: one right digest per left digest")
    return hash(level, np.concatenate([a, b], axis=1))


def commit_columns(level, columns, bit_reverse=True, return_nodes=False):
    """columns: (n_cols, N) natural-order columns of words.  Leaf j = hash of committed row j (natural row bitrev(j) with
    bit_reverse), node = merge.  Returns the root (digest_len,) uint64 (and `nodes`, (2N - 1, digest_len) root first in
    the layout of the reference's trees, when return_nodes)."""
    d = digest_len(level)
    cols = np.ascontiguousarray(columns, dtype=np.uint64)
    if cols.ndim != 2 or cols.shape[0] == 0:
        raise ValueError("commit_columns: columns is (n_cols, N) with at least one column")
    return _tree.commit_host(cols, d, np.uint64, return_nodes, lambda log2n, root, nodes: L.lib().lw_rpo_commit_columns(
        level, _vp(cols), cols.shape[0], log2n, 1 if bit_reverse else 0, root, nodes))


# ---- device-resident forms: torch int64 tensors holding the same words, 16-byte aligned
def permute_device(level, t_states, n, t_out=None, stream=None):
    """n states in t_states -> t_out (default: in place)"""
    t_out = t_states if t_out is None else t_out
    check(L.lib().lw_rpo_permute_device(level, _dp(t_states), n, _dp(t_out), _stream(stream)))
    return t_out


def hash_device(level, t_rows, n_rows, row_len, t_out, row_stride=0, stream=None):
    """n_rows rows of row_len words, row_stride words apart (0: dense) -> n_rows digests in t_out"""
    check(L.lib().lw_rpo_hash_device(level, _dp(t_rows) if row_len else None, n_rows, row_len, row_stride, _dp(t_out), _stream(stream)))
    return t_out


def merge_device(level, t_pairs, n, t_out, stream=None):
    """t_pairs: n pairs of adjacent digests (a level of `nodes` as it lies) -> their n parents in t_out"""
    return hash_device(level, t_pairs, n, 2 * digest_len(level), t_out, stream=stream)


def commit_columns_device(level, t_columns, n_cols, log2n, t_nodes, bit_reverse=True, col_stride=0, return_root=True, stream=None):
    """t_columns: n_cols columns of 2^log2n words, col_stride words apart (0: dense), e.g. the output of
    goldilocks.lde_device as it lies; t_nodes: (2 * 2^log2n - 1) x digest_len int64, the tree (for LEVEL_128 readable by
    merkle.open_trees_device as it is).  Returns the root (digest_len,) uint64 after synchronising the stream, or None
    (nothing waited for) with return_root=False."""
    return _tree.commit_device(digest_len(level), np.uint64, return_root, lambda root: L.lib().lw_rpo_commit_columns_device(
        level, _dp(t_columns), n_cols, col_stride, log2n, 1 if bit_reverse else 0, _dp(t_nodes), root, _stream(stream)))
