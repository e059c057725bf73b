"""Python restatement of the tail of the STARK prover's round 4 over host arrays, for the tests of stark_query.hip:
grinding (provers/stark/src/grinding.rs), MerkleTree::get_proof_by_pos (crypto/src/merkle_tree/merkle.rs:58-91,
utils.rs:7-21), fri::query_phase (provers/stark/src/fri/mod.rs:77-113) and open_trace_polys / open_composition_poly
(provers/stark/src/prover.rs:752-820)."""
import numpy as np

from oracle import oracle as O

PREFIX = bytes([0x01, 0x23, 0x45, 0x67, 0x89, 0xab, 0xcd, 0xed])


def inner_hash(seed, grinding_factor):
    return O.keccak256(PREFIX + bytes(seed) + bytes([grinding_factor]))


def is_valid_nonce(seed, nonce, grinding_factor, inner=None):
    inner = inner_hash(seed, grinding_factor) if inner is None else inner
    digest = O.keccak256(inner + int(nonce).to_bytes(8, "big"))
    return int.from_bytes(digest[:8], "big") < (1 << (64 - grinding_factor))


def smallest_nonce(seed, grinding_factor, first=0, last=2**64 - 1):
    inner = inner_hash(seed, grinding_factor)
    nonce = first
    while nonce <= last:
        if is_valid_nonce(seed, nonce, grinding_factor, inner):
            return nonce
        nonce += 1
    return None


def pointwise_nonces():
    """nonces that put a bit into every byte of bswap64(nonce), its low half included: every 2^k, every single byte 0xff,
    the three around 2^32, two patterns and the largest candidate, 2^64 - 2"""
    out = [1 << k for k in range(64)] + [0xff << (8 * j) for j in range(8)]
    out += [2**32 - 1, 2**32, 2**32 + 1, 2**63, 0x0123456789abcdef, 0xaaaaaaaaaaaaaaaa, 2**64 - 2]
    return sorted(set(out))


def bitrev(j, bits):
    return int(format(j, "0%db" % bits)[::-1], 2) if bits else 0


def merkle_path(nodes, pos):
    """nodes: (2 L - 1, 32) root first -> (log2 L, 32), bottom first"""
    nodes = np.asarray(nodes).reshape(-1, 32)
    i = pos + nodes.shape[0] // 2
    path = []
    while i != 0:
        path.append(nodes[i - 1 if i % 2 == 0 else i + 1])
        i = (i - 1) // 2 if i % 2 == 0 else i // 2
    return np.array(path, np.uint8).reshape(len(path), 32)


def fold_path(leaf_hash, pos, path):
    """the root a verifier computes from a leaf hash and its path"""
    h = bytes(leaf_hash)
    for node in path:
        h = O.keccak256(h + bytes(node)) if pos % 2 == 0 else O.keccak256(bytes(node) + h)
        pos //= 2
    return h


def open_tree(columns, nodes, log2_rows, rows_per_leaf, bit_reverse, pos):
    """-> (values (rows_per_leaf, n_cols, 4) or None, path): the committed rows of leaf pos and its path.
    columns: (n_cols, >= 2^log2_rows, 4) natural order, or None"""
    values = None
    if columns is not None:
        rows = [pos * rows_per_leaf + r for r in range(rows_per_leaf)]
        rows = [bitrev(j, log2_rows) if bit_reverse else j for j in rows]
        values = np.stack([np.stack([columns[c][row] for c in range(len(columns))]) for row in rows])
    return values, merkle_path(nodes, pos)


def fri_query_phase(layers, iotas):
    """layers: [(evaluation (domain, 4) as stored, i.e. bit-reversed; nodes (domain - 1, 32))] -> per iota
    (layers_evaluations_sym (n_layers, 4), [path per layer])"""
    out = []
    for iota in iotas:
        index, syms, paths = iota, [], []
        for evaluation, nodes in layers:
            syms.append(evaluation[index ^ 1])
            paths.append(merkle_path(nodes, index >> 1))
            index >>= 1
        out.append((np.stack(syms), paths))
    return out


def open_trace_polys(columns, nodes, log2_rows, iota):
    """columns (n_cols, 2^log2_rows, 4) natural order"""
    ev, proof = open_tree(columns, nodes, log2_rows, 1, True, 2 * iota)
    ev_sym, proof_sym = open_tree(columns, nodes, log2_rows, 1, True, 2 * iota + 1)
    return dict(evaluations=ev[0], evaluations_sym=ev_sym[0], proof=proof, proof_sym=proof_sym)


def open_composition_poly(parts, nodes, log2_rows, iota):
    """parts (n_parts, 2^log2_rows, 4) natural order; nodes over leaves of two consecutive bit-reversed rows"""
    proof = merkle_path(nodes, iota)
    ev = np.stack([p[bitrev(2 * iota, log2_rows)] for p in parts])
    ev_sym = np.stack([p[bitrev(2 * iota + 1, log2_rows)] for p in parts])
    return dict(evaluations=ev, evaluations_sym=ev_sym, proof=proof, proof_sym=proof)
