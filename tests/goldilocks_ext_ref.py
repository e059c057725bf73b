"""The quadratic extension of Goldilocks, Fp2 = F_p[t] / (t^2 - 7), and the prover steps of
lambda_elliptic_curves_amd/goldilocks_ext.py restated in Python integers (and numpy uint64 for the long vectors): what
the GPU tests compare against.  An element is a pair (c0, c1) of integers below p.  Follows extensions/quadratic.rs:79-118
over Goldilocks with non-residue 7, fri/fri_functions.rs:7-30 (fold) and fri/mod.rs:44-58, 115-141 (a layer)."""
import numpy as np

from tests import goldilocks_ref as G
from tests import rpo_ref

P = G.P
W = 7   # the non-residue: t^2 = 7
ZERO, ONE = (0, 0), (1, 0)


def elem(a):
    return (G.reduce_word(int(a[0])), G.reduce_word(int(a[1])))


def add(a, b):
    return ((a[0] + b[0]) % P, (a[1] + b[1]) % P)


def sub(a, b):
    return ((a[0] - b[0]) % P, (a[1] - b[1]) % P)


def mul(a, b):
    return ((a[0] * b[0] + W * a[1] * b[1]) % P, (a[0] * b[1] + a[1] * b[0]) % P)


def sqr(a):
    return mul(a, a)


def mul_base(a, b):
    return (a[0] * b % P, a[1] * b % P)


def inv(a):
    """conj(a) / norm(a); inv(0) = 0 (the library's convention, the reference's InvZeroError)"""
    ninv = pow((a[0] * a[0] - W * a[1] * a[1]) % P, P - 2, P)
    return (a[0] * ninv % P, -a[1] * ninv % P)


def power(a, e):
    r = ONE
    while e:
        if e & 1:
            r = mul(r, a)
        a = mul(a, a)
        e >>= 1
    return r


def horner(coeffs, x):
    """sum_i coeffs[i] x^i for base-field (or any u64) coefficients and x in Fp2"""
    acc = ZERO
    for c in reversed(coeffs):
        acc = mul(acc, x)
        acc = ((acc[0] + int(c)) % P, acc[1])
    return acc


def horner_ext(coeffs, x):
    """the same for Fp2 coefficients [(c0, c1), ...]"""
    acc = ZERO
    for c in reversed(coeffs):
        acc = add(mul(acc, x), c)
    return acc


# ---- numpy forms of the pointwise operations on planes of canonical words
def np_mul(a0, a1, b0, b1):
    m = G.np_mul
    return (G.np_add(m(a0, b0), m(m(a1, b1), np.uint64(W))), G.np_add(m(a0, b1), m(a1, b0)))


def np_mul_base(a0, a1, b):
    return G.np_mul(a0, b), G.np_mul(a1, b)


# ---- DEEP composition in evaluation form, from its definition
def deep_rows(cols, log2n, offset, root, points, weights, evals, rows=None):
    """out[i] = sum_j (sum_k weights[k][j] (cols[k][i] - evals[k][j])) / (x_i - points[j]), x_i = offset w^i, for the
    given rows (default: all 2^log2n).  cols: lists of base-field words; the tables hold Fp2 pairs."""
    w = G.root_of_unity(log2n, root)
    out = []
    for i in (range(1 << log2n) if rows is None else rows):
        x = offset % P * pow(w, i, P) % P
        total = ZERO
        for j, z in enumerate(points):
            num = ZERO
            for k, col in enumerate(cols):
                if weights[k][j] == ZERO:
                    continue
                num = add(num, mul(weights[k][j], sub((G.reduce_word(int(col[i])), 0), evals[k][j])))
            total = add(total, mul(num, inv(sub((x, 0), z))))
        out.append(total)
    return out


# ---- FRI over Fp2
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


def layer_evaluation(block, domain_size, offset, root=G.ROOT):
    """evaluate_offset_fft(p', 1, Some(domain_size), offset) in natural order: goldilocks_ref.lde of each plane"""
    L = domain_size.bit_length() - 1
    e0 = G.lde([c[0] for c in block], L, offset, root)
    e1 = G.lde([c[1] for c in block], L, offset, root)
    return list(zip(e0, e1))


def np_layer_evaluation(block, domain_size, offset, root=G.ROOT):
    """the same through the numpy transform -> (2, domain_size) uint64 planes"""
    planes = np.array([[c[0] for c in block], [c[1] for c in block]], np.uint64)
    return G.np_evaluate_fft(planes, offset, root, log2n=domain_size.bit_length() - 1)


def pair_index(j, domain_size):
    """leaf j commits (e[i], e[i + N/2]), i = bitrev(j) over log2(N) - 1 bits"""
    return G.bitrev(j, domain_size.bit_length() - 2) if domain_size > 2 else 0


def layer_rows(planes):
    """(2, N) planes of the evaluation -> the (N/2, 4) committed rows (a.c0, a.c1, b.c0, b.c1)"""
    planes = np.asarray(planes, np.uint64)
    n = planes.shape[1]
    idx = np.array([pair_index(j, n) for j in range(n // 2)], np.int64)
    return np.stack([planes[0, idx], planes[1, idx], planes[0, idx + n // 2], planes[1, idx + n // 2]], axis=1)


def layer_tree(level, planes):
    """nodes (N - 1, digest_len), root first: np_hash on the four-word rows, np_merge up"""
    return rpo_ref.np_trees(level, [layer_rows(planes)])[0]


def commit_phase(coeffs, number_layers, offset, domain_size, zetas, level, root=G.ROOT):
    """fri::commit_phase with the challenges taken from `zetas` -> (last value, [(planes, nodes)] per layer)"""
    zetas = list(zetas)
    poly, h, layers = list(coeffs), offset % P, []
    for _ in range(1, number_layers):
        h, domain_size = h * h % P, domain_size // 2
        poly = fold(poly, zetas.pop(0))
        planes = np_layer_evaluation(poly, domain_size, h, root)
        layers.append((planes, layer_tree(level, planes)))
    return fold(poly, zetas.pop(0))[0], layers
