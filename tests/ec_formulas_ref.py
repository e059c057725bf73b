"""Plain-integer reference of the group-law formulas of csrc/ec.cuh, for tests/test_gpu_ec_pointwise.py.

The complete formulas of Renes, Costello and Batina (Eurocrypt 2016, Algorithms 7, 8 and 9 for a = 0) are written out
operation by operation over Python integers, with b3 = 3b as a parameter.  They are polynomials in the coordinates, so
they are evaluated for ANY field elements, on the curve or not, and compared bit for bit with what the device returns.

A coordinate array holds Montgomery values: a stored word string is read as an integer s < p, stands for s R^-1 mod p,
goes through the polynomial and comes back as v R mod p (R = 2^(64 words)).  Fp2 is pairs of integers with u^2 = -1.

`lazy_shadow` re-evaluates the device-only branch of pt_add_mixed on integers that are NOT reduced where the device does
not reduce, and returns for each of its four product sites sum(a_q b_q) / p^2 as an exact fraction: how close the operands
come to the bound fe_dot was told (LAZY_BOUNDS).  `lazy_targets` searches inputs that drive each site to the top.
"""
import itertools
import random
from fractions import Fraction

import numpy as np

from oracle import bigint_def as D

OP_ADD, OP_ADD_MIXED, OP_DBL, OP_ADD_QUAD, OP_TO_AFFINE = range(5)   # lw_ec_op_t


# ---------------------------------------------------------------- the two coordinate fields
class Field:
    """Fp (elements: int) or Fp2 = Fp[u]/(u^2 + 1) (elements: (c0, c1))."""

    def __init__(self, p, fp2):
        self.p, self.fp2 = p, fp2
        self.zero = (0, 0) if fp2 else 0
        self.one = (1, 0) if fp2 else 1
        self.order = p * p if fp2 else p

    def add(self, a, b):
        p = self.p
        return ((a[0] + b[0]) % p, (a[1] + b[1]) % p) if self.fp2 else (a + b) % p

    def sub(self, a, b):
        p = self.p
        return ((a[0] - b[0]) % p, (a[1] - b[1]) % p) if self.fp2 else (a - b) % p

    def mul(self, a, b):
        p = self.p
        if self.fp2:
            return ((a[0] * b[0] - a[1] * b[1]) % p, (a[0] * b[1] + a[1] * b[0]) % p)
        return a * b % p

    def scale(self, a, k):
        """a times the base-field integer k"""
        p = self.p
        return (a[0] * k % p, a[1] * k % p) if self.fp2 else a * k % p

    def inv(self, a):
        p = self.p
        if self.fp2:
            n = pow(a[0] * a[0] + a[1] * a[1], -1, p)
            return (a[0] * n % p, -a[1] * n % p)
        return pow(a, -1, p)

    def pow(self, a, e):
        r = self.one
        while e:
            if e & 1:
                r = self.mul(r, a)
            a = self.mul(a, a)
            e >>= 1
        return r

    def elem(self, x):
        if self.fp2:
            return (x[0] % self.p, x[1] % self.p) if isinstance(x, tuple) else (x % self.p, 0)
        return x % self.p

    def root(self, w, k, rng):
        """one k-th root of w (k prime, w a k-th power): w^(1/k mod t) is right up to an element of the k-Sylow subgroup
        of order k^s (order - 1 = k^s t), which is small here and walked through."""
        s, t = 0, self.order - 1
        while t % k == 0:
            s, t = s + 1, t // k
        x = self.pow(w, pow(k, -1, t))
        while True:
            c = self.elem((rng.randrange(self.p), rng.randrange(self.p))) if self.fp2 else rng.randrange(1, self.p)
            g = self.pow(c, t)
            if s == 0 or self.pow(g, k ** (s - 1)) != self.one:
                break
        h = self.one
        for _ in range(k ** s):
            y = self.mul(x, h)
            if self.pow(y, k) == w:
                return y
            h = self.mul(h, g)
        raise ValueError("not a k-th power")


# ---------------------------------------------------------------- RCB16, a = 0, written out literally
def alg7_add(F, b3, P, Q):
    """Algorithm 7: complete projective addition."""
    X1, Y1, Z1 = P
    X2, Y2, Z2 = Q
    t0 = F.mul(X1, X2); t1 = F.mul(Y1, Y2); t2 = F.mul(Z1, Z2)
    t3 = F.add(X1, Y1); t4 = F.add(X2, Y2); t3 = F.mul(t3, t4)
    t4 = F.add(t0, t1); t3 = F.sub(t3, t4); t4 = F.add(Y1, Z1)
    X3 = F.add(Y2, Z2); t4 = F.mul(t4, X3); X3 = F.add(t1, t2)
    t4 = F.sub(t4, X3); X3 = F.add(X1, Z1); Y3 = F.add(X2, Z2)
    X3 = F.mul(X3, Y3); Y3 = F.add(t0, t2); Y3 = F.sub(X3, Y3)
    X3 = F.add(t0, t0); t0 = F.add(X3, t0); t2 = F.mul(b3, t2)
    Z3 = F.add(t1, t2); t1 = F.sub(t1, t2); Y3 = F.mul(b3, Y3)
    X3 = F.mul(t4, Y3); t2 = F.mul(t3, t1); X3 = F.sub(t2, X3)
    Y3 = F.mul(Y3, t0); t1 = F.mul(t1, Z3); Y3 = F.add(t1, Y3)
    t0 = F.mul(t0, t3); Z3 = F.mul(Z3, t4); Z3 = F.add(Z3, t0)
    return X3, Y3, Z3


def alg8_add_mixed(F, b3, P, Q):
    """Algorithm 8: complete mixed addition, Z2 = 1; Q = (X2, Y2) is not the identity."""
    X1, Y1, Z1 = P
    X2, Y2 = Q
    t0 = F.mul(X1, X2); t1 = F.mul(Y1, Y2); t3 = F.add(X2, Y2)
    t4 = F.add(X1, Y1); t3 = F.mul(t3, t4); t4 = F.add(t0, t1)
    t3 = F.sub(t3, t4); t4 = F.mul(Y2, Z1); t4 = F.add(t4, Y1)
    Y3 = F.mul(X2, Z1); Y3 = F.add(Y3, X1); X3 = F.add(t0, t0)
    t0 = F.add(X3, t0); t2 = F.mul(b3, Z1); Z3 = F.add(t1, t2)
    t1 = F.sub(t1, t2); Y3 = F.mul(b3, Y3); X3 = F.mul(t4, Y3)
    t2 = F.mul(t3, t1); X3 = F.sub(t2, X3); Y3 = F.mul(Y3, t0)
    t1 = F.mul(t1, Z3); Y3 = F.add(t1, Y3); t0 = F.mul(t0, t3)
    Z3 = F.mul(Z3, t4); Z3 = F.add(Z3, t0)
    return X3, Y3, Z3


def alg9_dbl(F, b3, P):
    """Algorithm 9: complete doubling."""
    X, Y, Z = P
    t0 = F.mul(Y, Y); Z3 = F.add(t0, t0); Z3 = F.add(Z3, Z3)
    Z3 = F.add(Z3, Z3); t1 = F.mul(Y, Z); t2 = F.mul(Z, Z)
    t2 = F.mul(b3, t2); X3 = F.mul(t2, Z3); Y3 = F.add(t0, t2)
    Z3 = F.mul(t1, Z3); t1 = F.add(t2, t2); t2 = F.add(t1, t2)
    t0 = F.sub(t0, t2); Y3 = F.mul(t0, Y3); Y3 = F.add(X3, Y3)
    t1 = F.mul(X, Y); X3 = F.mul(t0, t1); X3 = F.add(X3, X3)
    return X3, Y3, Z3


# ---------------------------------------------------------------- the six curve models of the device
class Model:
    """One curve as the device computes on it.  curve: LW_CURVE_* (= the oracle's id); model 1: its isomorphic model
    y^2 = x^3 + L^6 b under (x, y) -> (L^2 x, L^3 y).  b3: the field element 3b.  lazy: pt_add_mixed takes its
    unreduced-sum branch (the FpOps curves)."""

    def __init__(self, name, curve, model, b, l6=None):
        c = D.CURVES[curve]
        self.name, self.curve, self.model = name, curve, model
        self.p, self.fp2 = c.p, c.fp2
        self.F = Field(c.p, c.fp2)
        self.words = 6 if c.p == D.P_FP381 else 4                 # u64 words of a base-field element
        self.comps = 2 if c.fp2 else 1                            # base-field components of a coordinate
        self.R = 1 << (64 * self.words)
        self.Rinv = pow(self.R, -1, self.p)
        self.b = self.F.elem(b)
        self.b3 = self.F.scale(self.b, 3)
        self.l6 = l6                                              # model 1: L^6, else None
        self.lazy = not c.fp2
        self.coord_words = self.words * self.comps

    def __repr__(self):
        return self.name


def _curve_b(curve):
    b = D.CURVES[curve].b
    return b.tup()


def _models():
    ms = []
    fp381, fp254 = Field(D.P_FP381, False), Field(D.P_FP254, True)
    ms.append(Model("bls12_381_g1", 0, 0, _curve_b(0)))                        # b = 4, b3 = 12
    l6 = fp381.inv(6)                                                         # L^6 = 1/6: b' = 4/6 = 2/3, b3 = 2
    ms.append(Model("bls12_381_g1_iso", 0, 1, fp381.mul(l6, _curve_b(0)), l6))
    ms.append(Model("bn254_g1", 1, 0, _curve_b(1)))                            # b = 3, b3 = 9
    ms.append(Model("bn254_g2", 2, 0, _curve_b(2)))                            # b = 3/(9 + u)
    l6 = fp254.mul((9, 1), fp254.inv(_curve_b(2)))                            # L^6 = (9 + u)/b: b' = 9 + u, b3 = 27 + 3u
    ms.append(Model("bn254_g2_iso", 2, 1, fp254.mul(l6, _curve_b(2)), l6))
    ms.append(Model("bls12_381_g2", 3, 0, _curve_b(3)))                        # b = 4(1 + u)
    return ms


MODELS = _models()
assert MODELS[0].b3 == 12 and MODELS[1].b3 == 2 and MODELS[2].b3 == 9 and MODELS[4].b3 == (27, 3) and MODELS[5].b3 == (12, 12)


def iso_constants(m, seed=1):
    """(L^2, L^3) of model 1, derived from L^6 alone: a cube root and a square root of it.  Any pair (u2, u3) with
    u2^3 = u3^2 = L^6 is an isomorphism (x, y) -> (u2 x, u3 y) onto y^2 = x^3 + L^6 b (it is the standard one with
    u = u3/u2), so whichever roots come out map the group law onto the model's."""
    rng = random.Random(seed)
    return m.F.root(m.l6, 3, rng), m.F.root(m.l6, 2, rng)


# ---------------------------------------------------------------- stored (Montgomery) form
def from_stored(m, c):
    return tuple(x * m.Rinv % m.p for x in c) if m.fp2 else c * m.Rinv % m.p


def to_stored(m, c):
    return tuple(x * m.R % m.p for x in c) if m.fp2 else c * m.R % m.p


def stored_const(m, x):
    """the stored form of the field element x (an int, or a pair for Fp2)"""
    return to_stored(m, m.F.elem(x))


def stored_op(m, op, a, b=None):
    """One row of the seam on stored coordinates: a = (X, Y, Z), b = (X, Y, Z) / (x, y) / None -> stored (X, Y, Z)."""
    F = m.F
    if op == OP_ADD_MIXED and b == (F.zero, F.zero):
        return tuple(a)                                   # the identity row: the accumulation skips the formula
    if op == OP_TO_AFFINE:
        if a[2] == F.zero:
            return (F.zero, stored_const(m, 1), F.zero)
        X, Y, Z = (from_stored(m, c) for c in a)
        zi = F.inv(Z)
        return (to_stored(m, F.mul(X, zi)), to_stored(m, F.mul(Y, zi)), stored_const(m, 1))
    P = tuple(from_stored(m, c) for c in a)
    if op in (OP_ADD, OP_ADD_QUAD):
        r = alg7_add(F, m.b3, P, tuple(from_stored(m, c) for c in b))
    elif op == OP_ADD_MIXED:
        r = alg8_add_mixed(F, m.b3, P, tuple(from_stored(m, c) for c in b))
    elif op == OP_DBL:
        r = alg9_dbl(F, m.b3, P)
    else:
        raise ValueError(op)
    return tuple(to_stored(m, c) for c in r)


def pack_rows(m, rows):
    """rows of stored coordinates (ints, or pairs for Fp2) -> (n, coordinates * coord_words) uint64, reference layout:
    u64 words most significant first, c0 before c1."""
    ncoord = len(rows[0])
    nb = 8 * m.words
    buf = bytearray()
    for r in rows:
        for c in r:
            for v in (c if m.fp2 else (c,)):
                buf += v.to_bytes(nb, "big")
    out = np.frombuffer(bytes(buf), dtype=">u8").astype(np.uint64).reshape(len(rows), ncoord * m.coord_words)
    return np.ascontiguousarray(out)


def unpack_rows(m, arr):
    """the inverse of pack_rows"""
    arr = np.ascontiguousarray(arr, dtype=np.uint64)
    n = arr.shape[0]
    raw = arr.astype(">u8").tobytes()
    nb = 8 * m.words
    vals = [int.from_bytes(raw[i:i + nb], "big") for i in range(0, len(raw), nb)]
    per = len(vals) // n
    rows = []
    for i in range(n):
        v = vals[i * per:(i + 1) * per]
        rows.append(tuple((v[2 * j], v[2 * j + 1]) for j in range(per // 2)) if m.fp2 else tuple(v))
    return rows


# ---------------------------------------------------------------- operands where field arithmetic goes wrong
def edge_values(p, words, seed):
    """The edge set E of one base-field coordinate, as stored integers < p."""
    rng = random.Random(seed)
    n32 = 2 * words
    R = 1 << (64 * words)
    e = [0, 1, 2, p - 1, p - 2, (p - 1) // 2, (p + 1) // 2, R % p]
    for j in range(1, n32):
        e += [1 << (32 * j), (1 << (32 * j)) - 1, p - (1 << (32 * j))]
    low_zero = rng.randrange(p) >> 32 << 32
    top = rng.randrange(p >> (32 * (n32 - 1)))                      # below p's top limb: the value stays below p
    mid_ones = (top << (32 * (n32 - 1))) | (((1 << (32 * (n32 - 2))) - 1) << 32) | rng.randrange(1 << 32)
    e += [low_zero, mid_ones]
    assert all(0 <= v < p for v in e)
    return e


def inverse_operands(p, words, seed, n_top=2000):
    """Non-zero operands of an inversion: E, 2^k, 2^k +- 1 and p - 2^k for every bit k, and n_top values whose top two
    32-bit limbs are p's and whose lower limbs are random or zero."""
    rng = random.Random(seed)
    n32 = 2 * words
    vals = [v for v in edge_values(p, words, seed) if v]
    for k in range(p.bit_length()):
        vals += [v for v in ((1 << k), (1 << k) + 1, (1 << k) - 1, p - (1 << k)) if 0 < v < p]
    top = p >> (32 * (n32 - 2)) << (32 * (n32 - 2))
    while n_top:
        low = 0
        for j in range(n32 - 2):
            low |= (rng.randrange(1 << 32) if rng.random() < 0.5 else 0) << (32 * j)
        if 0 < top + low < p:
            vals.append(top + low)
            n_top -= 1
    return vals


# ---------------------------------------------------------------- the lazy branch of pt_add_mixed, unreduced
# fe_dot's KSUM at the four product sites: mul_k<4>, dot2_k<1 + 2 KY>, dot2_k<KZ + 3 KY>, dot2_k<2 KZ + 3>
# with KZ = 2 for Fp381 (z3 unreduced) else 1 and KY = 2 for the isomorphic model of BLS12-381 G1 (b3 y3 = y3 + y3 unreduced) else 1
LAZY_BOUNDS = {
    "bls12_381_g1": {"mul4": 4, "xo": 3, "yo": 5, "zo": 7},
    "bls12_381_g1_iso": {"mul4": 4, "xo": 5, "yo": 8, "zo": 7},
    "bn254_g1": {"mul4": 4, "xo": 3, "yo": 4, "zo": 5},
}
SITES = ("mul4", "xo", "yo", "zo")


def lazy_shadow(m, px, py, pz, qx, qy):
    """pt_add_mixed's device branch on the stored integers, unreduced where the device leaves a sum unreduced: add_nr,
    t0x3, t4, z3 (Fp381), y3 (b3 = 2) and 2p - t4.  Returns ({site: sum a_q b_q / p^2}, stored (X3, Y3, Z3)): the
    Montgomery reduction of a sum S gives S R^-1 mod p."""
    assert m.lazy
    p, Ri = m.p, m.Rinv
    wide, b3_is_2 = p == D.P_FP381, m.b3 == 2
    mm = lambda a, b: a * b * Ri % p
    t0, t1 = mm(px, qx), mm(py, qy)
    s_t3 = (qx + qy) * (px + py)                       # mul_k<4>: both sums unreduced
    t3 = (s_t3 * Ri - (t0 + t1)) % p
    t4 = mm(qy, pz) + py                               # < 2p
    y3 = (mm(qx, pz) + px) % p
    t0x3 = 3 * t0                                      # < 3p
    t2 = m.b3 * pz % p                                 # mul_b3 is reduced additions
    z3 = t1 + t2 if wide else (t1 + t2) % p
    t1 = (t1 - t2) % p
    y3 = 2 * y3 if b3_is_2 else m.b3 * y3 % p
    n4 = 2 * p - t4                                    # fe_neg_raw_2p: in (0, 2p]
    s_xo = t3 * t1 + n4 * y3
    s_yo = t1 * z3 + y3 * t0x3
    s_zo = z3 * t4 + t0x3 * t3
    pp = p * p
    ratios = {"mul4": Fraction(s_t3, pp), "xo": Fraction(s_xo, pp), "yo": Fraction(s_yo, pp), "zo": Fraction(s_zo, pp)}
    return ratios, (s_xo * Ri % p, s_yo * Ri % p, s_zo * Ri % p)


N_KEEP = 64


def lazy_targets(m, seed=2024):
    """For each product site of the lazy branch, N_KEEP inputs (px, py, pz, qx, qy), stored, that drive its unreduced sum
    to the top of its range, best first, and the opposite corner (t4 = 0: fe_neg_raw_2p returns exactly 2p).

    The intermediates a site needs near their maxima are solved for with modular inverses (mm(a, b) = t has
    b = t R / a) and fixed a few units below p.  What cannot be fixed is searched in two independent stages instead of
    one: stage 1 walks the small offsets or a free coordinate for the intermediate that depends on (py, qy, pz) only,
    stage 2 walks px (or solves the remaining 2 x 2 linear system) on the best of stage 1; a few thousand shadow
    evaluations per stage cover what a joint search would need their product for."""
    rng = random.Random(seed)
    p, R, Ri = m.p, m.R, m.Rinv
    inv = lambda x: pow(x, -1, p)
    mm = lambda a, b: a * b * Ri % p
    mdiv = lambda t, a: t * R * inv(a) % p             # the b with mm(a, b) = t
    b3 = m.b3
    wide, b3_is_2 = p == D.P_FP381, b3 == 2
    ratio = lambda site, c: lazy_shadow(m, *c)[0][site]
    best = lambda site, cands: sorted(set(cands), key=lambda c: -ratio(site, c))[:N_KEEP]
    out = {}

    # mul_k<4>: (qx + qy)(px + py), all four a few units below p
    out["mul4"] = best("mul4", [(p - i, p - j, rng.randrange(p), p - k, p - l)
                                for i, j, k, l in itertools.product((1, 2, 3), (1, 2, 3), (1, 2, 3), (1, 2, 3))])

    # zo = z3 t4 + t0x3 t3: t1, t2 = b3 pz, py and t0 fixed below p; q.y p.z (stage 1) and t3 (stage 2) searched
    s1 = []
    for a, b, e in itertools.product(range(1, 14), repeat=3):
        py, pz = p - a, (p - e) * inv(b3) % p
        qy = mdiv(p - b, py)
        z3 = (p - b) + (p - e) if wide else (2 * p - b - e) % p
        s1.append((z3 * (mm(qy, pz) + py), py, qy, pz))
    cands = []
    for _, py, qy, pz in sorted(s1, reverse=True)[:4]:
        for _ in range(1500):
            px = rng.randrange(1, p)
            cands.append((px, py, pz, mdiv(p - rng.randrange(1, 4), px), qy))
    out["zo"] = best("zo", cands)

    # yo = t1' z3 + y3 t0x3 with t1' = t1 - t2, z3 = t1 + t2: (t1, t2) from a small grid (stage 1), t0 fixed, y3 searched over px
    s1 = []
    for a, b, e, hi in itertools.product(range(1, 8), range(1, 14), range(1, 14), (0, 1)):
        t1, t2 = p - b, (p - e if hi else e)
        py, pz = p - a, t2 * inv(b3) % p
        z3 = t1 + t2 if wide else (t1 + t2) % p
        s1.append((((t1 - t2) % p) * z3, py, mdiv(t1, py), pz))
    cands = []
    for _, py, qy, pz in sorted(s1, reverse=True)[:4]:
        for _ in range(1500):
            px = rng.randrange(1, p)
            cands.append((px, py, pz, mdiv(p - rng.randrange(1, 4), px), qy))
    out["yo"] = best("yo", cands)

    # xo = t3 t1' + (2p - t4) y3: t4 = q.y p.z + p.y a few units above 0, t1' searched over p.z (stage 1); then y3 and
    # t3 = mm(qx, py) + mm(qy, px) are two linear equations in (px, qx)
    s1 = []
    for _ in range(3000):
        py, pz = rng.randrange(1, 4), rng.randrange(1, p)
        qy = mdiv(py + rng.randrange(1, 4), pz)            # q.y p.z != p.y keeps the linear system of stage 2 regular
        s1.append(((mm(py, qy) - b3 * pz) % p, py, qy, pz))
    cands = []
    for _, py, qy, pz in sorted(s1, reverse=True)[:4]:
        al, be, ga = pz * Ri % p, py * Ri % p, qy * Ri % p
        for d, e in itertools.product(range(1, 6), repeat=2):
            w = p - d if b3_is_2 else (p - d) * inv(b3) % p
            den = (be - ga * al) % p
            if den == 0:
                continue
            qx = (-e - ga * w) * inv(den) % p
            cands.append(((w - al * qx) % p, py, pz, qx, qy))
    out["xo"] = best("xo", cands)

    # the opposite corner: p.y = 0 and q.y p.z = 0 give t4 = 0, and 2p - t4 = 2p exactly; q is never (0, 0)
    r = lambda: rng.randrange(1, p)
    out["corner"] = [(0, 0, 0, 1, 0), (0, 0, 0, p - 1, 0), (r(), 0, r(), r(), 0), (r(), 0, 0, r(), r()), (p - 1, 0, p - 1, p - 1, 0),
                     (p - 1, 0, 0, p - 1, p - 1), (0, 0, r(), r(), 0), (r(), 0, 0, 0, r())]
    return out
