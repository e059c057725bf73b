"""Rescue Prime Optimized over Goldilocks restated in Python integers (and in numpy uint64 for the batches and trees):
what the tests of lambda_elliptic_curves_amd/rpo.py compare against.  Follows RescuePrimeOptimized of the reference
(crypto/src/hash/rescue_prime/rescue_prime_optimized.rs: permutation :192-202, hash :205-230; utils.rs:8-21
bytes_to_field_elements) and ePrint 2022/1577.  The round constants are derived here once more from SHAKE256, the MDS
circulants are written out from their first rows."""
import hashlib

import numpy as np

from tests import goldilocks_ref as G

P = G.P
ALPHA = 7
ALPHA_INV = 10540996611094048183
assert ALPHA * ALPHA_INV % (P - 1) == 1
N_ROUNDS = 7
LEVEL_128, LEVEL_160 = 0, 1
# level -> (security level, m, capacity, first row of the circulant M[i][j] = v[(j - i) mod m])
PARAMS = {
    LEVEL_128: (128, 12, 4, [7, 23, 8, 26, 13, 10, 9, 7, 6, 22, 21, 8]),
    LEVEL_160: (160, 16, 6, [256, 2, 1 << 30, 1 << 11, 1 << 24, 1 << 7, 8, 16, 1 << 19, 1 << 22, 1, 1 << 28, 1, 1 << 10, 2, 1 << 13]),
}


def width(level):
    return PARAMS[level][1]


def capacity(level):
    return PARAMS[level][2]


def rate(level):
    return PARAMS[level][1] - PARAMS[level][2]


def digest_len(level):
    return rate(level) // 2


def round_constants(level):
    sec, m, cap, _ = PARAMS[level]
    count = 2 * m * N_ROUNDS
    stream = hashlib.shake_256(("RPO(%d,%d,%d,%d)" % (P, m, cap, sec)).encode()).digest(9 * count)
    return [int.from_bytes(stream[9 * i:9 * i + 9], "little") % P for i in range(count)]


RC = {level: round_constants(level) for level in PARAMS}


# ---- Python integers
def mds(level, s):
    _, m, _, v = PARAMS[level]
    return [sum(v[(j - i) % m] * s[j] for j in range(m)) % P for i in range(m)]


def permute(level, state):
    """permutation(): any u64 words in (read mod p), canonical residues out"""
    m = width(level)
    s = [w % P for w in state]
    assert len(s) == m
    rc = RC[level]
    for r in range(N_ROUNDS):
        s = mds(level, s)
        s = [pow((x + rc[2 * m * r + j]) % P, ALPHA, P) for j, x in enumerate(s)]
        s = mds(level, s)
        s = [pow((x + rc[2 * m * r + m + j]) % P, ALPHA_INV, P) for j, x in enumerate(s)]
    return s


def hash(level, seq):
    m, cap, rt = width(level), capacity(level), rate(level)
    seq = [w % P for w in seq]
    s = [0] * m
    if len(seq) % rt:
        s[0] = 1
    full = len(seq) // rt
    for b in range(full):
        s[cap:] = seq[b * rt:(b + 1) * rt]
        s = permute(level, s)
    last = len(seq) % rt
    if last:
        s[cap:] = seq[full * rt:] + [1] + [0] * (rt - last - 1)
        s = permute(level, s)
    return s[cap:cap + rt // 2]


def bytes_to_field_elements(data):
    out = []
    for at in range(0, len(data), 7):
        chunk = bytes(data[at:at + 7])
        if len(chunk) < 7:
            chunk += b"\x01"
        out.append(int.from_bytes(chunk, "little") % P)
    return out


def hash_bytes(level, data):
    return hash(level, bytes_to_field_elements(data))


def sbox_inv_chain(x):
    """x^(1/7) by the 72-product addition chain of the kernels; acc(b, t, n) = b^(2^n) * t"""
    acc = lambda b, t, n: pow(b, 1 << n, P) * t % P
    t1 = x * x % P
    t2 = t1 * t1 % P
    t3 = acc(t2, t2, 3)
    t4 = acc(t3, t3, 6)
    t5 = acc(t4, t4, 12)
    t6 = acc(t5, t3, 6)
    t7 = acc(t6, t6, 31)
    a = t7 * t7 % P * t6 % P
    a = pow(a, 4, P)
    return a * t1 % P * t2 % P * x % P


# ---- numpy uint64: (n, m) states, one permutation per row
def np_pow_small(x, e):
    r, b = None, x
    while e:
        if e & 1:
            r = b if r is None else G.np_mul(r, b)
        e >>= 1
        if e:
            b = G.np_mul(b, b)
    return r


_S32, _EPS = np.uint64(32), np.uint64(G.EPS)


def np_mds(level, s):
    """out[i] = sum_k v[k] s[(i + k) mod m] over the integers in 32-bit halves (the sums stay below 2^63 for any u64
    words, PARAMS: sum v < 2^31), then one reduction of lo + 2^32 hi; checked against mds() by tests/test_rpo_cpu.py"""
    v = PARAMS[level][3]
    lo, hi = s & _EPS, s >> _S32
    a, b = np.zeros_like(s), np.zeros_like(s)
    for k, vk in enumerate(v):
        a += np.roll(lo, -k, axis=1) * np.uint64(vk)
        b += np.roll(hi, -k, axis=1) * np.uint64(vk)
    x_lo = a + (b << _S32)
    x_hi = (b >> _S32) + (x_lo < a).astype(np.uint64)
    # x_lo + 2^64 x_hi with x_hi < 2^32: 2^64 = EPS mod p, and x_hi EPS < 2^64
    t1 = (x_hi << _S32) - x_hi
    t2 = x_lo + t1
    t2 = np.where(t2 < t1, t2 + _EPS, t2)
    return G.np_reduce(t2)


def np_sbox_inv(x):
    """x^(1/7) by the 72-product chain (sbox_inv_chain)"""
    def acc(b, t, n):
        for _ in range(n):
            b = G.np_mul(b, b)
        return G.np_mul(b, t)
    t1 = G.np_mul(x, x)
    t2 = G.np_mul(t1, t1)
    t3 = acc(t2, t2, 3)
    t4 = acc(t3, t3, 6)
    t5 = acc(t4, t4, 12)
    t6 = acc(t5, t3, 6)
    t7 = acc(t6, t6, 31)
    a = acc(t7, t6, 1)
    a = G.np_mul(a, a)
    a = G.np_mul(a, a)
    return G.np_mul(G.np_mul(a, G.np_mul(t1, t2)), x)


def np_permute(level, states):
    m = width(level)
    s = G.np_reduce(np.asarray(states, np.uint64).reshape(-1, m))
    rc = np.array(RC[level], np.uint64).reshape(2 * N_ROUNDS, 1, m)
    for r in range(N_ROUNDS):
        s = np_pow_small(G.np_add(np_mds(level, s), rc[2 * r]), ALPHA)
        s = np_sbox_inv(G.np_add(np_mds(level, s), rc[2 * r + 1]))
    return s


def np_hash(level, rows):
    """rows: (n_rows, row_len) -> (n_rows, digest_len)"""
    m, cap, rt = width(level), capacity(level), rate(level)
    rows = G.np_reduce(np.asarray(rows, np.uint64))
    n, length = rows.shape
    s = np.zeros((n, m), np.uint64)
    if length % rt:
        s[:, 0] = 1
        pad = np.zeros((n, rt - length % rt), np.uint64)
        pad[:, 0] = 1
        rows = np.concatenate([rows, pad], axis=1)
    for b in range(rows.shape[1] // rt):
        s[:, cap:] = rows[:, b * rt:(b + 1) * rt]
        s = np_permute(level, s)
    return s[:, cap:cap + rt // 2].copy()


def np_merge(level, left, right):
    return np_hash(level, np.concatenate([left, right], axis=1))


def np_trees(level, row_sets):
    """row_sets: matrices (N, n_cols_k) of committed rows, one per tree, all with the same N -> their nodes arrays
    (2 N - 1, digest_len), root first (merkle_tree/utils.rs layout).  The node levels of all the trees go through one
    batched permutation per level."""
    n = row_sets[0].shape[0]
    bits = n.bit_length() - 1
    d, k = digest_len(level), len(row_sets)
    nodes = np.zeros((k, 2 * n - 1, d), np.uint64)
    for t, rows in enumerate(row_sets):
        assert rows.shape[0] == n
        nodes[t, n - 1:] = np_hash(level, rows)
    for lvl in range(bits, 0, -1):
        first = (1 << lvl) - 1
        ch = nodes[:, first:first + (1 << lvl)]
        parents = np_merge(level, ch[:, 0::2].reshape(-1, d), ch[:, 1::2].reshape(-1, d))
        nodes[:, first // 2:first] = parents.reshape(k, -1, d)
    return [nodes[t] for t in range(k)]


def committed_rows(columns, bit_reverse=True):
    """(n_cols, N) natural-order columns -> (N, n_cols) rows in committed order"""
    cols = np.asarray(columns, np.uint64)
    n = cols.shape[1]
    rows = cols.T
    return rows[[G.bitrev(j, n.bit_length() - 1) for j in range(n)]] if bit_reverse else rows


def np_tree(level, columns, bit_reverse=True):
    """columns: (n_cols, N) natural order -> nodes (2 N - 1, digest_len), root first"""
    return np_trees(level, [committed_rows(columns, bit_reverse)])[0]


def edge_states(level):
    """states for the permutation's edge test: all zero, all p - 1, the non-canonical all 2^64 - 1 and all p, every EDGE
    operand of goldilocks_ref broadcast, and the EDGE list rotated through the positions"""
    m = width(level)
    states = [[0] * m, [P - 1] * m, [(1 << 64) - 1] * m, [P] * m]
    states += [[v] * m for v in G.EDGE]
    states += [[G.EDGE[(j + k) % len(G.EDGE)] for j in range(m)] for k in range(len(G.EDGE))]
    return states
