"""The quartic extension of Mersenne31 and the prover steps that run in it, restated from the definitions in plain integers
on top of circle_ref and monolith_ref: CM31 = F_p[i] / (i^2 + 1), QM31 = CM31[u] / (u^2 - (2 + i)) (Degree2ExtensionField /
Degree4ExtensionField of math/src/field/fields/mersenne31/extensions.rs), the circle basis over QM31, the DEEP quotients by
the line through P and its conjugate, the circle FRI fold in evaluation form, the layer tree and a commit phase with a
callable transcript.  An element is a tuple (c0, c1, c2, c3) = (c0 + c1 i) + (c2 + c3 i) u of canonical residues."""
import functools

import numpy as np

from . import circle_ref as CR
from . import monolith_ref as MR

P = CR.P
ZERO, ONE = (0, 0, 0, 0), (1, 0, 0, 0)
HALF = 1 << 30   # 2 * 2^30 = 2^31 = 1


def elem(words):
    """four words, read the way circle.py reads any u32"""
    return tuple(CR.reduce_word(w) for w in words)


def embed(a):
    return (a % P, 0, 0, 0)


# ---- CM31
def c_mul(a, b):
    return ((a[0] * b[0] - a[1] * b[1]) % P, (a[0] * b[1] + a[1] * b[0]) % P)


def c_inv(a):
    n = CR.inv((a[0] * a[0] + a[1] * a[1]) % P)
    return (a[0] * n % P, -a[1] * n % P)


def c_nonresidue(a):
    """(a, b) -> (2 + i)(a + b i) = (2a - b, 2b + a): mul_fp2_by_nonresidue"""
    return ((2 * a[0] - a[1]) % P, (2 * a[1] + a[0]) % P)


# ---- QM31
def add(a, b):
    return tuple((x + y) % P for x, y in zip(a, b))


def sub(a, b):
    return tuple((x - y) % P for x, y in zip(a, b))


def neg(a):
    return tuple(-x % P for x in a)


def mul(a, b):
    a0, a1, b0, b1 = a[:2], a[2:], b[:2], b[2:]
    a0b0, a1b1 = c_mul(a0, b0), c_mul(a1, b1)
    nr = c_nonresidue(a1b1)
    cross = c_mul(((a0[0] + a1[0]) % P, (a0[1] + a1[1]) % P), ((b0[0] + b1[0]) % P, (b0[1] + b1[1]) % P))
    return ((a0b0[0] + nr[0]) % P, (a0b0[1] + nr[1]) % P, (cross[0] - a0b0[0] - a1b1[0]) % P, (cross[1] - a0b0[1] - a1b1[1]) % P)


def sqr(a):
    return mul(a, a)


def mul_base(a, b):
    return tuple(x * b % P for x in a)


def inv(a):
    """0 -> 0"""
    a0, a1 = a[:2], a[2:]
    s0, nr = c_mul(a0, a0), c_nonresidue(c_mul(a1, a1))
    norm = ((s0[0] - nr[0]) % P, (s0[1] - nr[1]) % P)
    if norm == (0, 0):
        return ZERO
    n = c_inv(norm)
    return c_mul(a0, n) + c_mul(((-a1[0]) % P, (-a1[1]) % P), n)


def conj(a):
    """sigma: u -> -u, fixes CM31"""
    return (a[0], a[1], -a[2] % P, -a[3] % P)


def times_i(a):
    return (-a[1] % P, a[0], -a[3] % P, a[2])


def times_u(a):
    """(a0 + a1 u) u = (2 + i) a1 + a0 u"""
    return c_nonresidue(a[2:]) + (a[0], a[1])


def combine_planes(v):
    """v[0] + i v[1] + u v[2] + i u v[3] for four QM31 values"""
    return add(add(v[0], times_i(v[1])), add(times_u(v[2]), times_i(times_u(v[3]))))


def plane_weights(w):
    """the weight rows of an Fp4 column passed as its four planes: w (1, i, u, iu)"""
    return [list(w), [times_i(x) for x in w], [times_u(x) for x in w], [times_i(times_u(x)) for x in w]]


def circle_point(t):
    """a point of the circle over QM31 from a parameter t with 1 + t^2 != 0"""
    t2 = sqr(t)
    d = inv(add(ONE, t2))
    return mul(sub(ONE, t2), d), mul(add(t, t), d)


# ---- out-of-domain evaluation
def basis_value(k, x, y):
    """circle_ref.basis_value over QM31"""
    v = y if k & 1 else ONE
    k >>= 1
    while k:
        if k & 1:
            v = mul(v, x)
        x = sub(mul_base(sqr(x), 2), ONE)
        k >>= 1
    return v


def evaluate(coeffs, point):
    x, y = point
    total = ZERO
    for k, c in enumerate(coeffs):
        total = add(total, mul_base(basis_value(k, x, y), CR.reduce_word(c)))
    return total


# ---- DEEP quotients
def deep_quotients(cols, log2n, points, weights, evals):
    """cols: n_cols lists of 2^log2n words; points: [(X, Y)]; weights, evals: [k][j] -> the 2^log2n values of t_out"""
    dom = CR.coset_points(log2n)
    out = []
    for i, (xi, yi) in enumerate(dom):
        total = ZERO
        for j, (X, Y) in enumerate(points):
            sX, sY = conj(X), conj(Y)
            cj = sub(sY, Y)
            num = ZERO
            for k, col in enumerate(cols):
                v, w = evals[k][j], weights[k][j]
                a = sub(conj(v), v)
                b = sub(mul(v, cj), mul(a, Y))
                term = sub(sub(mul_base(cj, CR.reduce_word(col[i])), mul_base(a, yi)), b)
                num = add(num, mul(w, term))
            D = add(add(mul_base(sub(Y, sY), xi), mul_base(sub(sX, X), yi)), sub(mul(X, sY), mul(Y, sX)))
            assert D[0] == 0 and D[1] == 0 and D != ZERO
            total = add(total, mul(num, inv(D)))
        out.append(total)
    return out


# ---- circle FRI
def fold_twiddles(log2m, first):
    """t_i, i < M/2: y of the coset of size M for the fold from the circle to the line, else x of the coset of size 2M"""
    if first:
        return [q[1] for q in CR.coset_points(log2m)[: (1 << log2m) // 2]]
    return [q[0] for q in CR.coset_points(log2m + 1)[: (1 << log2m) // 2]]


def fold(v, zeta, first):
    M = len(v)
    tw = fold_twiddles(M.bit_length() - 1, first)
    out = []
    for i in range(M // 2):
        a, b = v[i], v[M - 1 - i]
        out.append(mul_base(add(add(a, b), mul(mul_base(zeta, CR.inv(tw[i])), sub(a, b))), HALF))
    return out


def fold_coeffs(c, zeta):
    return [add(c[2 * m], mul(zeta, c[2 * m + 1])) for m in range(len(c) // 2)]


def pair_columns(v):
    """the eight columns of M/2 words a layer of M values is committed as"""
    M = len(v)
    return [[v[i][e] for i in range(M // 2)] for e in range(4)] + [[v[M - 1 - i][e] for i in range(M // 2)] for e in range(4)]


def layer_tree(rounds, v):
    """-> the nodes, root first, of the Monolith tree over the M/2 leaves (v[i], v[M-1-i])"""
    return MR.np_tree(rounds, np.array(pair_columns(v), np.uint32), False)


def commit_phase(v, number_layers, rounds, challenge):
    """-> (last layer, [(layer values, nodes)]); challenge(prev_root_or_None) -> zeta"""
    layers, prev = [], None
    for k in range(number_layers):
        v = fold(v, challenge(prev), k == 0)
        if k + 1 < number_layers:
            nodes = layer_tree(rounds, v)
            layers.append((v, nodes))
            prev = nodes[0]
    return v, layers


# ---- the same in numpy, for the sizes of the GPU tests: an array of elements is (4, n) uint64 of canonical residues
_P = np.uint64(P)


def np_elems(words):
    """(4, n) words -> canonical residues"""
    w = np.asarray(words).astype(np.uint64) & np.uint64(0xFFFFFFFF)
    return ((w & _P) + (w >> np.uint64(31))) % _P


def np_of(elems):
    """[(c0, c1, c2, c3)] -> (4, n)"""
    return np.array(elems, np.uint64).reshape(-1, 4).T.copy()


def elems_of(a):
    return [tuple(int(v) for v in col) for col in np.asarray(a).T]


def _cmul(a0, a1, b0, b1):
    return (a0 * b0 % _P + (_P - a1 * b1 % _P)) % _P, (a0 * b1 % _P + a1 * b0 % _P) % _P


def np_mul(a, b):
    """(4, n) x (4, n) or (4, 1)"""
    p0, p1 = _cmul(a[0], a[1], b[0], b[1])
    q0, q1 = _cmul(a[2], a[3], b[2], b[3])
    r0, r1 = _cmul((a[0] + a[2]) % _P, (a[1] + a[3]) % _P, (b[0] + b[2]) % _P, (b[1] + b[3]) % _P)
    n0, n1 = (2 * q0 + _P - q1) % _P, (2 * q1 + q0) % _P
    return np.stack([(p0 + n0) % _P, (p1 + n1) % _P, (r0 + 2 * _P - p0 - q0) % _P, (r1 + 2 * _P - p1 - q1) % _P])


def np_add(a, b):
    return (a + b) % _P


def np_sub(a, b):
    return (a + _P - b) % _P


def np_mul_base(a, b):
    return a * (np.asarray(b, np.uint64) % _P) % _P


def np_inv_base(a):
    r, b, e = np.ones_like(a), a.copy(), P - 2
    while e:
        if e & 1:
            r = r * b % _P
        b = b * b % _P
        e >>= 1
    return r


def np_inv(a):
    s0, s1 = _cmul(a[0], a[1], a[0], a[1])
    t0, t1 = _cmul(a[2], a[3], a[2], a[3])
    n0, n1 = (s0 + 2 * _P - (2 * t0 + _P - t1) % _P) % _P, (s1 + _P - (2 * t1 + t0) % _P) % _P
    ni = np_inv_base((n0 * n0 % _P + n1 * n1 % _P) % _P)
    i0, i1 = n0 * ni % _P, (_P - n1) % _P * ni % _P
    lo, hi = _cmul(a[0], a[1], i0, i1), _cmul((_P - a[2]) % _P, (_P - a[3]) % _P, i0, i1)
    return np.stack([lo[0], lo[1], hi[0], hi[1]])


def _col(e):
    return np.array(e, np.uint64).reshape(4, 1)


def np_evaluate(coeffs, point):
    """2^L words at (X, Y): the pairs that differ in bit j fold under the factor of bit j"""
    x, y = point
    c = np_elems(coeffs)
    v = np.stack([c, np.zeros_like(c), np.zeros_like(c), np.zeros_like(c)])
    f = y
    for j in range(len(coeffs).bit_length() - 1):
        v = np_add(v[:, 0::2], np_mul(v[:, 1::2], _col(f)))
        f = x if j == 0 else sub(mul_base(sqr(f), 2), ONE)
    return elems_of(v)[0]


@functools.lru_cache(maxsize=None)
def np_coset(log2n):
    """(x, y) of the standard coset as two uint64 arrays"""
    pts = CR.coset_points(log2n)
    return np.array([q[0] for q in pts], np.uint64), np.array([q[1] for q in pts], np.uint64)


def np_deep_quotients(cols, log2n, points, weights, evals):
    """cols: (n_cols, N) words -> (4, N)"""
    xs, ys = np_coset(log2n)
    c = np_elems(cols)
    out = np.zeros((4, 1 << log2n), np.uint64)
    for j, (X, Y) in enumerate(points):
        sX, sY = conj(X), conj(Y)
        cj = sub(sY, Y)
        num = np.zeros_like(out)
        for k in range(len(cols)):
            v, w = evals[k][j], weights[k][j]
            a = sub(conj(v), v)
            b = sub(mul(v, cj), mul(a, Y))
            term = np_sub(np_sub(np_mul_base(_col(cj), c[k]), np_mul_base(_col(a), ys)), _col(b))
            num = np_add(num, np_mul(term, _col(w)))
        D = np_add(np_add(np_mul_base(_col(sub(Y, sY)), xs), np_mul_base(_col(sub(sX, X)), ys)), _col(sub(mul(X, sY), mul(Y, sX))))
        out = np_add(out, np_mul(num, np_inv(D)))
    return out


def np_fold(v, zeta, first):
    """(4, M) -> (4, M / 2)"""
    M = v.shape[1]
    lg = M.bit_length() - 1
    t = (np_coset(lg)[1] if first else np_coset(lg + 1)[0])[: M // 2]
    a, b = v[:, : M // 2], v[:, ::-1][:, : M // 2]
    z = np_mul_base(_col(zeta), np_inv_base(t))
    return np_mul_base(np_add(np_add(a, b), np_mul(np_sub(a, b), z)), HALF)


def np_pair_columns(v):
    M = v.shape[1]
    return np.concatenate([v[:, : M // 2], v[:, ::-1][:, : M // 2]]).astype(np.uint32)
