"""The quartic extension of BabyBear, Fp4 = F_p[x] / (x^4 + 11), and the prover steps of
lambda_elliptic_curves_amd/babybear_ext.py restated in Python integers on UNSTORED values (plain residues below p; numpy
uint64 for the long vectors): what the GPU tests compare against.  An element is a tuple (c0, c1, c2, c3).  Follows
fields/fft_friendly/quartic_babybear.rs, fri/fri_functions.rs:7-30 (fold) and fri/mod.rs:44-58, 115-141 (a layer).  The
device keeps STORED words (v 2^32 mod p): store / unstore and their numpy forms sit at the boundary."""
import numpy as np

from oracle import oracle as O
from tests import keccak_tree_ref as K

P = 2013265921
BETA = 11   # x^4 = -11
R = 1 << 32
R_INV = pow(R, -1, P)
ZERO, ONE = (0, 0, 0, 0), (1, 0, 0, 0)
# the edge set of stored words
EDGE = [0, 1, 2, P - 1, P - 2, (P - 1) // 2, (P + 1) // 2, R % P]
EDGE_B = [0, 1, P - 1, (P + 1) // 2]


def store(v):
    return int(v) % P * R % P


def unstore(w):
    return int(w) * R_INV % P


def store_elem(a):
    return tuple(store(c) for c in a)


def unstore_elem(a):
    return tuple(unstore(c) for c in a)


def np_store(v):
    return ((np.asarray(v, np.uint64) << np.uint64(32)) % np.uint64(P)).astype(np.uint32)


def np_unstore(w):
    return np.asarray(w, np.uint64) * np.uint64(R_INV) % np.uint64(P)


def add(a, b):
    return tuple((x + y) % P for x, y in zip(a, b))


def sub(a, b):
    return tuple((x - y) % P for x, y in zip(a, b))


def mul(a, b):
    a0, a1, a2, a3 = a
    b0, b1, b2, b3 = b
    return ((a0 * b0 - BETA * (a1 * b3 + a2 * b2 + a3 * b1)) % P,
            (a0 * b1 + a1 * b0 - BETA * (a2 * b3 + a3 * b2)) % P,
            (a0 * b2 + a1 * b1 + a2 * b0 - BETA * a3 * b3) % P,
            (a0 * b3 + a1 * b2 + a2 * b1 + a3 * b0) % P)


def sqr(a):
    return mul(a, a)


def mul_base(a, b):
    return tuple(c * b % P for c in a)


def inv(a):
    """a(-x) (b0 - b2 y) / c with b0 + b2 y = a(x) a(-x) in F_p[y] / (y^2 + 11), y = x^2, and c = b0^2 + 11 b2^2 its norm;
    inv(0) = 0 (the library's convention, the reference's error)"""
    a0, a1, a2, a3 = a
    b0 = (a0 * a0 + BETA * (2 * a1 * a3 - a2 * a2)) % P
    b2 = (2 * a0 * a2 - a1 * a1 + BETA * a3 * a3) % P
    c_inv = pow((b0 * b0 + BETA * b2 * b2) % P, P - 2, P)
    b0, b2 = b0 * c_inv % P, b2 * c_inv % P
    return ((a0 * b0 + BETA * a2 * b2) % P, (-a1 * b0 - BETA * a3 * b2) % P, (-a0 * b2 + a2 * b0) % P, (a1 * b2 - a3 * b0) % P)


def power(a, e):
    r = ONE
    while e:
        if e & 1:
            r = mul(r, a)
        a = mul(a, a)
        e >>= 1
    return r


def horner(coeffs, x):
    """sum_i coeffs[i] x^i for base-field coefficients and x in Fp4"""
    acc = ZERO
    for c in reversed(coeffs):
        acc = mul(acc, x)
        acc = ((acc[0] + int(c)) % P,) + acc[1:]
    return acc


def horner_ext(coeffs, x):
    """the same for Fp4 coefficients"""
    acc = ZERO
    for c in reversed(coeffs):
        acc = add(mul(acc, x), c)
    return acc


def np_horner(coeffs, x, block=1024):
    """horner() for a long column of residues: the sums of `block` coefficients against the table 1, x, ..., x^(block - 1)
    in numpy, then Horner over the blocks under x^block"""
    c = np.asarray(coeffs, np.uint64)
    c = np.concatenate([c, np.zeros(-len(c) % block, np.uint64)]).reshape(-1, block)
    table = [ONE]
    for _ in range(block - 1):
        table.append(mul(table[-1], x))
    xb = mul(table[-1], x)
    sums = [(c * np.array([t[e] for t in table], np.uint64) % np.uint64(P)).sum(axis=1) % np.uint64(P) for e in range(4)]
    acc = ZERO
    for i in range(c.shape[0] - 1, -1, -1):
        acc = add(mul(acc, xb), tuple(int(s[i]) for s in sums))
    return acc


# ---- numpy forms on (4, n) uint64 planes of residues
def _m(a, b):
    return a * b % np.uint64(P)


def np_mul(a, b):
    p, beta = np.uint64(P), np.uint64(BETA)
    neg = lambda s: (p - s % p) * beta   # -11 s, below 2^35
    return np.stack([(_m(a[0], b[0]) + neg(_m(a[1], b[3]) + _m(a[2], b[2]) + _m(a[3], b[1]))) % p,
                     (_m(a[0], b[1]) + _m(a[1], b[0]) + neg(_m(a[2], b[3]) + _m(a[3], b[2]))) % p,
                     (_m(a[0], b[2]) + _m(a[1], b[1]) + _m(a[2], b[0]) + neg(_m(a[3], b[3]))) % p,
                     (_m(a[0], b[3]) + _m(a[1], b[2]) + _m(a[2], b[1]) + _m(a[3], b[0])) % p])


def np_mul_base(a, b):
    return np.stack([_m(a[e], b) for e in range(4)])


def planes_of(elems):
    return np.array([[e[k] for e in elems] for k in range(4)], np.uint64).reshape(4, len(elems))


def elems_of(planes):
    return [tuple(int(v) for v in col) for col in np.asarray(planes).T]


# ---- the domain: the library's primitive 2^k-th root (babybear.rs: the 2^24-th root 21, squared down)
def root_of_unity(log2n):
    return pow(21, 1 << (24 - log2n), P)


def bitrev(i, bits):
    return K.bitrev(i, bits)


def lde(coeffs, log2n, offset):
    """the values of sum_i coeffs[i] X^i at offset w^i, i < 2^log2n, from the definition (small sizes)"""
    w = root_of_unity(log2n)
    out = []
    for i in range(1 << log2n):
        x, acc = offset * pow(w, i, P) % P, 0
        for c in reversed(coeffs):
            acc = (acc * x + int(c)) % P
        out.append(acc)
    return out


def np_lde(planes, log2n, offset):
    """evaluate_offset_fft(p, 1, Some(2^log2n), offset) of every row of `planes` (residues) -> (rows, 2^log2n) residues,
    through the compiled BabyBear transform on stored words"""
    off = np.array([store(offset)], np.uint32)
    rows = [O.evaluate_fft(O.F_BABYBEAR_U32, np_store(row), 1, 1 << log2n, off) if np.any(row) else np.zeros(1 << log2n, np.uint32)
            for row in np.asarray(planes, np.uint64)]
    return np.stack([np_unstore(r) for r in rows])


# ---- DEEP composition in evaluation form, from its definition
def deep_rows(cols, log2n, offset, points, weights, evals, rows=None):
    """out[i] = sum_j (sum_k weights[k][j] (cols[k][i] - evals[k][j])) / (x_i - points[j]), x_i = offset w^i, for the
    given rows (default: all 2^log2n).  cols: lists of base-field residues; the tables hold Fp4 tuples."""
    w = root_of_unity(log2n)
    out = []
    for i in (range(1 << log2n) if rows is None else rows):
        x = offset % P * pow(w, i, P) % P
        total = ZERO
        for j, z in enumerate(points):
            num = ZERO
            for k, col in enumerate(cols):
                if weights[k][j] == ZERO:
                    continue
                num = add(num, mul(weights[k][j], sub((int(col[i]), 0, 0, 0), evals[k][j])))
            total = add(total, mul(num, inv(sub((x, 0, 0, 0), z))))
        out.append(total)
    return out


# ---- FRI over Fp4
def folded_block(n_coeffs):
    return max(2, 1 << max((n_coeffs + 1) // 2 - 1, 0).bit_length())


def fold(coeffs, zeta):
    """p'_i = 2 (c_2i + zeta c_2i+1) as the zero-padded block of folded_block(len) elements"""
    n = len(coeffs)
    out = []
    for i in range((n + 1) // 2):
        v = coeffs[2 * i]
        if 2 * i + 1 < n:
            v = add(v, mul(zeta, coeffs[2 * i + 1]))
        out.append(add(v, v))
    return out + [ZERO] * (folded_block(n) - len(out))


def layer_evaluation(block, domain_size, offset):
    """evaluate_offset_fft(p', 1, Some(domain_size), offset) in natural order, from the definition"""
    L = domain_size.bit_length() - 1
    return list(zip(*[lde([c[e] for c in block], L, offset) for e in range(4)]))


def np_layer_evaluation(block, domain_size, offset):
    """the same through the compiled transform -> (4, domain_size) uint64 planes of residues"""
    return np_lde(planes_of(block), domain_size.bit_length() - 1, offset)


def pair_index(j, domain_size):
    """leaf j commits (e[i], e[i + N/2]), i = bitrev(j) over log2(N) - 1 bits"""
    return bitrev(j, domain_size.bit_length() - 2) if domain_size > 2 else 0


def layer_rows(planes):
    """(4, N) planes of the evaluation -> the (N/2, 8) committed rows (a.c0 .. a.c3, b.c0 .. b.c3)"""
    planes = np.asarray(planes)
    n = planes.shape[1]
    idx = np.array([pair_index(j, n) for j in range(n // 2)], np.int64)
    return np.concatenate([planes[:, idx], planes[:, idx + n // 2]]).T


def leaf_hash(stored_row):
    """Keccak-256 of the eight stored words of a row, each big-endian"""
    return O.keccak256(b"".join(int(w).to_bytes(4, "big") for w in stored_row))


def layer_tree(planes):
    """nodes (N - 1, 32) uint8, root first, over the stored words of the rows of layer_rows"""
    rows = np_store(layer_rows(planes))
    return O.merkle_commit_columns_babybear(np.ascontiguousarray(rows.T), bit_reverse=False)


def commit_phase(coeffs, number_layers, offset, domain_size, zetas):
    """fri::commit_phase with the challenges taken from `zetas` -> (last value, [(planes, nodes)] per layer)"""
    zetas = list(zetas)
    poly, h, layers = list(coeffs), offset % P, []
    for _ in range(1, number_layers):
        h, domain_size = h * h % P, domain_size // 2
        poly = fold(poly, zetas.pop(0))
        planes = np_layer_evaluation(poly, domain_size, h)
        layers.append((planes, layer_tree(planes)))
    return fold(poly, zetas.pop(0))[0], layers
