"""Multilinear tables and the sumcheck round in plain Python integers: the restatement that the device code is compared
with (DenseMultilinearPolynomial::evaluate / fix_variables, math/src/polynomial/dense_multilinear_poly.rs).

A table T of 2^n values is a polynomial in x_0 .. x_{n-1} with x_0 on the most significant bit of the index.  Fld(p)
computes on residues; Fld(p, montgomery=True) on STORED values a R mod p (R = 2^256) with the product A B R^-1, which is
what the library keeps in memory, so its results can be compared bit for bit."""

P_STARK252 = 0x800000000000011000000000000000000000000000000000000000000000001
P_FR381 = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001
MODULI = {"stark252": P_STARK252, "fr381": P_FR381}


class Fld:
    def __init__(self, p, montgomery=False):
        self.p = p
        self.rinv = pow(1 << 256, -1, p) if montgomery else 1
        self.one = (1 << 256) % p if montgomery else 1

    def mul(self, a, b):
        return a * b * self.rinv % self.p

    def elem(self, v):
        """the integer v as an element"""
        return v * self.one % self.p

    def plain(self, a):
        """the residue an element stands for"""
        return a * self.rinv % self.p


def chis(F, r):
    """the reference's table: chis[i] = prod_j eq(r_j, bit_{n-1-j}(i)), built with its loop"""
    c = [F.one] * (1 << len(r))
    size = 1
    for rj in r:
        size *= 2
        for i in range(size - 1, 0, -2):
            s = c[i // 2]
            c[i] = F.mul(s, rj)
            c[i - 1] = (s - c[i]) % F.p
    return c


def evaluate(F, T, r):
    assert len(T) == 1 << len(r)
    c = chis(F, r)
    return sum(F.mul(t, w) for t, w in zip(T, c)) % F.p


def fix_variables(F, T, r):
    """T'[j] = sum_b eq(r, b) T[b 2^(n-t) + j], one variable at a time from the top: lo + r (hi - lo)"""
    T = list(T)
    for rj in r:
        h = len(T) // 2
        assert h >= 1
        T = [(T[j] + F.mul(rj, (T[j + h] - T[j]) % F.p)) % F.p for j in range(h)]
    return T


def round_poly(F, tables):
    """[g(0) .. g(K)], g(t) = sum_{j<h} prod_k (T_k[j] + t (T_k[j+h] - T_k[j]))"""
    K, h = len(tables), len(tables[0]) // 2
    assert h >= 1 and all(len(T) == 2 * h for T in tables)
    g = [0] * (K + 1)
    for j in range(h):
        v = [T[j] for T in tables]
        d = [(T[j + h] - T[j]) % F.p for T in tables]
        for t in range(K + 1):
            prod = v[0]
            for k in range(1, K):
                prod = F.mul(prod, v[k])
            g[t] += prod
            v = [(a + b) % F.p for a, b in zip(v, d)]
    return [x % F.p for x in g]


def cube_sum(F, tables):
    total = 0
    for j in range(len(tables[0])):
        prod = tables[0][j]
        for T in tables[1:]:
            prod = F.mul(prod, T[j])
        total += prod
    return total % F.p


def prove(F, tables, challenge):
    """the honest prover: -> (claimed_sum, rounds, point, final_evals); challenge maps a round's values to the next r"""
    tables = [list(T) for T in tables]
    rounds, point = [], []
    while len(tables[0]) > 1:
        g = round_poly(F, tables)
        r = challenge(g)
        rounds.append(g)
        point.append(r)
        tables = [fix_variables(F, T, [r]) for T in tables]
    return (rounds[0][0] + rounds[0][1]) % F.p, rounds, point, [T[0] for T in tables]


def interpolate(p, ys, x):
    """the polynomial through (i, ys[i]), i = 0 .. len(ys) - 1, at x; residues"""
    total = 0
    for i, yi in enumerate(ys):
        num, den = 1, 1
        for m in range(len(ys)):
            if m != i:
                num = num * (x - m) % p
                den = den * (i - m) % p
        total += yi * num * pow(den, -1, p)
    return total % p


def verify(F, claimed_sum, rounds, point, final_evals):
    """g_i(0) + g_i(1) = g_{i-1}(r_{i-1}) (the claimed sum first), and prod_k final_k = g_n(r_n) at the end"""
    p = F.p
    if len(rounds) != len(point) or not rounds:
        return False
    expect = F.plain(claimed_sum)
    for g, r in zip(rounds, point):
        if len(g) != len(final_evals) + 1:
            return False
        ys = [F.plain(v) for v in g]
        if (ys[0] + ys[1]) % p != expect:
            return False
        expect = interpolate(p, ys, F.plain(r))
    prod = 1
    for v in final_evals:
        prod = prod * F.plain(v) % p
    return prod == expect
