"""Big-integer restatement of the Starknet Poseidon hash (crypto/src/hash/poseidon/mod.rs) and of the Merkle trees built
on it (crypto/src/merkle_tree/backends/field_element.rs:53-76 TreePoseidon, field_element_vector.rs:61-85
BatchPoseidonTree, utils.rs:24-71 node layout).  Independent of the library and of tools/gen_poseidon_consts.py: the keys
are derived here again from the SHA-256 rule.  Values are canonical Python integers; to_elems / from_elems convert to
the library's boundary layout (4 x u64, most significant limb first, Montgomery form)."""
import hashlib

import numpy as np

P = 2**251 + 17 * 2**192 + 1
R = 2**256
R_INV = pow(R, -1, P)
N_ROUNDS, HALF_FULL, N_PARTIAL = 91, 4, 83

KEYS = [[int(hashlib.sha256(("Hades" + str(3 * i + j)).encode()).hexdigest(), 16) % P for j in range(3)] for i in range(N_ROUNDS)]


def mix(s):
    t = s[0] + s[1] + s[2]
    return [(t + 2 * s[0]) % P, (t - 2 * s[1]) % P, (t - 3 * s[2]) % P]


def permute(state):
    """hades_permutation, the three-add schedule: every round adds its three keys; rounds 0-3 and 87-90 cube all three
    words, rounds 4-86 cube word 2 only"""
    s = [x % P for x in state]
    for i in range(N_ROUNDS):
        s = [(s[j] + KEYS[i][j]) % P for j in range(3)]
        if i < HALF_FULL or i >= HALF_FULL + N_PARTIAL:
            s = [pow(x, 3, P) for x in s]
        else:
            s[2] = pow(s[2], 3, P)
        s = mix(s)
    return s


def hash2(x, y):
    return permute([x, y, 2])[0]


def hash_single(x):
    return permute([x, 0, 1])[0]


def hash_many(values):
    v = list(values) + [1]
    if len(v) % 2:
        v.append(0)
    s = [0, 0, 0]
    for k in range(0, len(v), 2):
        s = permute([s[0] + v[k], s[1] + v[k + 1], s[2]])
    return s[0]


def tree_nodes(leaves):
    """nodes of the tree over the hashed leaves (a power of two of them): inner nodes root first, then the leaves"""
    n = len(leaves)
    assert n and n & (n - 1) == 0
    nodes = [0] * (n - 1) + list(leaves)
    for k in range(n - 2, -1, -1):
        nodes[k] = hash2(nodes[2 * k + 1], nodes[2 * k + 2])
    return nodes


def bitrev(i, bits):
    return int(format(i, "0%db" % bits)[::-1], 2) if bits else 0


def commit_columns(columns, leaf_many, bit_reverse):
    """columns: n_cols lists of 2^k canonical integers -> nodes (integers)"""
    n = len(columns[0])
    bits = n.bit_length() - 1
    rows = [[col[bitrev(i, bits) if bit_reverse else i] for col in columns] for i in range(n)]
    if leaf_many:
        leaves = [hash_many(r) for r in rows]
    else:
        assert len(columns) == 1
        leaves = [hash_single(r[0]) for r in rows]
    return tree_nodes(leaves)


# ---- boundary layout
def to_elems(values):
    """canonical integers -> (len, 4) uint64, MS limb first, Montgomery form"""
    out = np.zeros((len(values), 4), np.uint64)
    for i, x in enumerate(values):
        m = x % P * R % P
        for k in range(4):
            out[i, 3 - k] = (m >> (64 * k)) & 0xffffffffffffffff
    return out


def raw_ints(elems):
    """(…, 4) uint64 MS limb first -> the raw 256-bit integers (Montgomery residues, not converted)"""
    a = np.asarray(elems, dtype=np.uint64).reshape(-1, 4)
    return [(int(r[0]) << 192) | (int(r[1]) << 128) | (int(r[2]) << 64) | int(r[3]) for r in a]


def from_elems(elems):
    """(…, 4) uint64 -> canonical integers (out of Montgomery form)"""
    return [m * R_INV % P for m in raw_ints(elems)]
