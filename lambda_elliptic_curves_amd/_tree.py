"""The commit bodies of the algebraic hashes (poseidon, rpo, pedersen, monolith), once: each module passes the length and
dtype of its digest and a closure that makes the C call in the hash's own argument order."""
import numpy as np

from ._lib import host_ptr as _vp
from .errors import InputError, check


def commit_host(cols, digest_len, dtype, return_nodes, call):
    """cols: (n_cols, N, ...); call(log2n, root, nodes_or_None) -> status.  Returns root, or (root, nodes)."""
    n = cols.shape[1]
    log2n = n.bit_length() - 1
    if n == 0 or (1 << log2n) != n:
        raise InputError(f"Input length is {n}, which is not a power of two")
    root = np.zeros(digest_len, dtype)
    nodes = np.zeros((2 * n - 1, digest_len), dtype) if return_nodes else None
    check(call(log2n, _vp(root), _vp(nodes)))
    return (root, nodes) if return_nodes else root


def commit_device(digest_len, dtype, return_root, call):
    """call(root_or_None) -> status.  Returns the root, or None (nothing waited for) with return_root=False."""
    root = np.zeros(digest_len, dtype) if return_root else None
    check(call(_vp(root)))
    return root
