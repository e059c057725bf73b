"""Monolith over Mersenne31 restated in Python integers (and in numpy uint64 for the batches and trees): what the tests of
lambda_elliptic_curves_amd/monolith.py compare against.  Follows MonolithMersenne31<WIDTH, NUM_FULL_ROUNDS> of the
reference (crypto/src/hash/monolith/mod.rs: constants :47-55, Bars tables :57-89, permutation :91-102, Concrete
:105-174; utils.rs).  Bars is the table form the reference defines.  The two hashing modes are the ones Plonky3 builds
from the permutation for Mersenne31, PaddingFreeSponge<16, 8, 8> and TruncatedPermutation<2, 8, 16>, as include/lw_hip.h
specifies them."""
import hashlib

import numpy as np

P = (1 << 31) - 1
WIDTHS = (8, 12, 16, 20, 24)
NUM_BARS = 8
RATE, DIGEST, SPONGE_WIDTH = 8, 8, 16
CIRC16 = [61402, 17845, 26798, 59689, 12021, 40901, 41351, 27521, 56951, 12034, 53865, 43244, 7454, 33823, 28750, 1108]


def reduce_word(w):
    """a u32 read mod p"""
    return int(w) % P


# ---- constants (mod.rs:47-55, 109-116, 152-174; utils.rs:12-55)
class _Shake:
    """little-endian u32 words of a SHAKE128 stream"""

    def __init__(self, seed):
        self.seed, self.at, self.buf = seed, 0, b""

    def u32(self):
        if 4 * self.at + 4 > len(self.buf):
            self.buf = hashlib.shake_128(self.seed).digest(max(1024, 2 * len(self.buf)))
        v = int.from_bytes(self.buf[4 * self.at:4 * self.at + 4], "little")
        self.at += 1
        return v


def _seed(width, rounds):
    return b"Monolith" + bytes([width, rounds + 1]) + P.to_bytes(4, "little")


_CONSTS = {}


def constants(width, rounds):
    """-> (round constants: rounds rows of width words, the matrix of Concrete: width rows of width words)"""
    assert width in WIDTHS and 1 <= rounds <= 15
    if (width, rounds) in _CONSTS:
        return _CONSTS[(width, rounds)]
    sh = _Shake(_seed(width, rounds) + bytes([8, 8, 8, 7]))
    rc = []
    for _ in range(rounds):
        row = []
        while len(row) < width:
            v = sh.u32()
            if v < P:
                row.append(v)
        rc.append(row)
    if width == 16:
        mds = [[CIRC16[(j - i) % 16] for j in range(16)] for i in range(16)]   # the first row rotated right i times
    else:
        sh = _Shake(_seed(width, rounds) + bytes([16, 15]) + b"MDS")
        x_mask, y_mask = (1 << 22) - 1, P >> 2
        ys = []
        for _ in range(width):
            y = sh.u32() & y_mask
            while any((r & x_mask) == (y & x_mask) for r in ys):
                y = sh.u32() & y_mask
            ys.append(y)
        mds = [[pow((x & x_mask) + y, P - 2, P) for y in ys] for x in ys]
    _CONSTS[(width, rounds)] = (rc, mds)
    return rc, mds


# ---- Bars: the tables as the reference builds them (mod.rs:57-89)
def s_box(y):
    rot = lambda v, k: ((v << k) | (v >> (8 - k))) & 0xFF
    return rot(y ^ ((~rot(y, 1) & 0xFF) & rot(y, 2) & rot(y, 3)), 1)


def final_s_box(y):
    assert y >> 7 == 0
    r1 = ((y >> 6) | (y << 1)) & 0xFF
    r2 = ((y >> 5) | (y << 2)) & 0xFF
    tmp = (y ^ ((~r1 & 0xFF) & r2)) & 0x7F
    return ((tmp >> 6) | (tmp << 1)) & 0x7F


LOOKUP1 = np.array([(s_box(i >> 8) << 8) | s_box(i & 0xFF) for i in range(1 << 16)], np.uint64)
LOOKUP2 = np.array([(final_s_box(i >> 8) << 8) | s_box(i & 0xFF) for i in range(1 << 15)], np.uint64)


def bar(x):
    """one word of Bars, x in [0, p]"""
    return int(LOOKUP2[x >> 16]) << 16 | int(LOOKUP1[x & 0xFFFF])


# ---- Python integers
def bars(s):
    return [bar(x) for x in s[:NUM_BARS]] + list(s[NUM_BARS:])


def bricks(s):
    return [s[0]] + [(s[i] + s[i - 1] * s[i - 1]) % P for i in range(1, len(s))]


def concrete(s, mds):
    return [sum(m * x for m, x in zip(row, s)) % P for row in mds]


def permute(width, rounds, state):
    """permutation(): any u32 words in (read mod p), canonical residues out"""
    rc, mds = constants(width, rounds)
    s = [reduce_word(w) for w in state]
    assert len(s) == width
    s = concrete(s, mds)
    for r in range(rounds):
        s = concrete(bricks(bars(s)), mds)
        s = [(x + c) % P for x, c in zip(s, rc[r])]
    return concrete(bricks(bars(s)), mds)


def hash(rounds, seq):
    """PaddingFreeSponge<16, 8, 8>: every chunk of up to 8 words overwrites the front of the state; no padding"""
    s = [0] * SPONGE_WIDTH
    for at in range(0, len(seq), RATE):
        chunk = [reduce_word(w) for w in seq[at:at + RATE]]
        s[:len(chunk)] = chunk
        s = permute(SPONGE_WIDTH, rounds, s)
    return s[:DIGEST]


def compress(rounds, left, right):
    """TruncatedPermutation<2, 8, 16>"""
    assert len(left) == len(right) == DIGEST
    return permute(SPONGE_WIDTH, rounds, list(left) + list(right))[:DIGEST]


# ---- numpy uint64: (n, width) states, one permutation per row
_P64 = np.uint64(P)


def np_reduce(words):
    return np.asarray(words, np.uint64) % _P64


def np_bars(s):
    """s in [0, p]"""
    out = s.copy()
    b = s[:, :NUM_BARS]
    out[:, :NUM_BARS] = (LOOKUP2[(b >> np.uint64(16)).astype(np.int64)] << np.uint64(16)) | LOOKUP1[(b & np.uint64(0xFFFF)).astype(np.int64)]
    return out


def np_bricks(s):
    out = s.copy()
    out[:, 1:] = (s[:, 1:] + s[:, :-1] * s[:, :-1] % _P64) % _P64
    return out


def np_concrete(s, mds):
    m = np.array(mds, np.uint64)
    return (s[:, None, :] * m[None, :, :] % _P64).sum(axis=2) % _P64   # products below 2^62, at most 24 residues summed


def np_permute(width, rounds, states):
    rc, mds = constants(width, rounds)
    s = np_reduce(np.asarray(states).reshape(-1, width))
    s = np_concrete(s, mds)
    for r in range(rounds):
        s = (np_concrete(np_bricks(np_bars(s)), mds) + np.array(rc[r], np.uint64)) % _P64
    return np_concrete(np_bricks(np_bars(s)), mds).astype(np.uint32)


def np_hash(rounds, rows):
    """rows: (n_rows, row_len) -> (n_rows, 8)"""
    rows = np_reduce(rows)
    n, length = rows.shape
    s = np.zeros((n, SPONGE_WIDTH), np.uint64)
    for at in range(0, length, RATE):
        chunk = rows[:, at:at + RATE]
        s[:, :chunk.shape[1]] = chunk
        s = np_permute(SPONGE_WIDTH, rounds, s).astype(np.uint64)
    return s[:, :DIGEST].astype(np.uint32)


def np_compress(rounds, left, right):
    both = np.concatenate([np.asarray(left).reshape(-1, DIGEST), np.asarray(right).reshape(-1, DIGEST)], axis=1)
    return np_permute(SPONGE_WIDTH, rounds, both)[:, :DIGEST].copy()


def bitrev(j, bits):
    return int(format(j, "0%db" % bits)[::-1], 2) if bits else 0


def committed_rows(columns, bit_reverse=True):
    """(n_cols, N) natural-order columns -> (N, n_cols) rows in committed order"""
    cols = np.asarray(columns)
    n = cols.shape[1]
    rows = cols.T
    return rows[[bitrev(j, n.bit_length() - 1) for j in range(n)]] if bit_reverse else rows


def np_trees(rounds, row_sets):
    """row_sets: matrices (N, n_cols_k) of committed rows, one per tree, all with the same N -> their nodes arrays
    (2 N - 1, 8) uint32, root first (merkle_tree/utils.rs layout): leaf = hash of the row, node = compress.  The levels of
    all the trees go through one batched permutation per level."""
    n = row_sets[0].shape[0]
    bits = n.bit_length() - 1
    k = len(row_sets)
    nodes = np.zeros((k, 2 * n - 1, DIGEST), np.uint32)
    for t, rows in enumerate(row_sets):
        assert rows.shape[0] == n
        nodes[t, n - 1:] = np_hash(rounds, rows)
    for lvl in range(bits, 0, -1):
        first = (1 << lvl) - 1
        ch = nodes[:, first:first + (1 << lvl)]
        parents = np_compress(rounds, ch[:, 0::2].reshape(-1, DIGEST), ch[:, 1::2].reshape(-1, DIGEST))
        nodes[:, first // 2:first] = parents.reshape(k, -1, DIGEST)
    return [nodes[t] for t in range(k)]


def np_tree(rounds, columns, bit_reverse=True):
    """columns: (n_cols, N) natural order -> nodes (2 N - 1, 8), root first"""
    return np_trees(rounds, [committed_rows(columns, bit_reverse)])[0]


def bars_words():
    """words to put in front of Bars: the edge words, then every value of every byte lane (the 7-bit top lane included)
    with the other lanes all zeros and all ones"""
    words = [0, P, P - 1, 1, 1 << 30, 0x7F000000, 0x00FFFFFF]
    for shift, count in ((0, 256), (8, 256), (16, 256), (24, 128)):
        lane = (count - 1) << shift
        words += [v << shift for v in range(count)] + [(P & ~lane) | (v << shift) for v in range(count)]
    return words


def edge_states(width):
    """all 0, all p, all p - 1, all 2^31, all 2^32 - 1, and a one at every position"""
    states = [[v] * width for v in (0, P, P - 1, 1 << 31, 0xFFFFFFFF)]
    states += [[1 if j == k else 0 for j in range(width)] for k in range(width)]
    return states
