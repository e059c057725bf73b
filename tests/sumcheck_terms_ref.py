"""The sumcheck over an eq-weighted sum of products in plain Python integers, built on tests/multilinear_ref.py: the round
by its definition, an honest prover and a verifier.

The claim is sum_x E(x) * sum_t c_t * prod_{m in S_t} T_m(x) over the cube, E the table of eq(tau, .) or absent.  A term is
(c, (m, ...)): a coefficient (None is one) and the indices of the tables it multiplies.  Values are elements of a
multilinear_ref.Fld, so with montgomery=True they are the stored values of the library and compare bit for bit."""
from tests import multilinear_ref as M


def degree(terms, has_eq):
    return max(len(idx) for _, idx in terms) + (1 if has_eq else 0)


def bracket(F, terms, vals):
    """sum_t c_t prod_{m in S_t} vals[m]"""
    total = 0
    for c, idx in terms:
        prod = vals[idx[0]]
        for m in idx[1:]:
            prod = F.mul(prod, vals[m])
        total += prod if c is None else F.mul(c, prod)
    return total % F.p


def round_poly(F, tables, terms, eq=None):
    """[g(0) .. g(D)], g(u) = sum_{j<h} E_j(u) sum_t c_t prod_{m in S_t} T_m,j(u), X_j(u) = X[j] + u (X[j+h] - X[j])"""
    h = len(tables[0]) // 2
    every = list(tables) + ([eq] if eq is not None else [])
    assert h >= 1 and all(len(T) == 2 * h for T in every)
    D = degree(terms, eq is not None)
    p, rinv = F.p, F.rinv
    g = []
    for u in range(D + 1):   # column by column: X(u) for all j at once (u is a small integer: no Montgomery factor)
        at = [[(a + u * (b - a)) % p for a, b in zip(T[:h], T[h:])] for T in every]
        total = [0] * h
        for c, idx in terms:
            prod = at[idx[0]]
            for m in idx[1:]:
                prod = [x * y * rinv % p for x, y in zip(prod, at[m])]
            if c is not None:
                prod = [c * x * rinv % p for x in prod]
            total = [x + y for x, y in zip(total, prod)]
        if eq is not None:
            total = [e * (x % p) * rinv % p for e, x in zip(at[-1], total)]
        g.append(sum(total) % p)
    return g


def cube_sum(F, tables, terms, eq=None):
    total = 0
    for j in range(len(tables[0])):
        b = bracket(F, terms, [T[j] for T in tables])
        total += F.mul(eq[j], b) if eq is not None else b
    return total % F.p


def prove(F, tables, terms, challenge, eq=None):
    """the honest prover -> (claimed_sum, rounds, point, final_evals); final_evals holds every table's value at the point,
    the eq table's last"""
    every = [list(T) for T in tables] + ([list(eq)] if eq is not None else [])
    k = len(tables)
    rounds, point = [], []
    while len(every[0]) > 1:
        g = round_poly(F, every[:k], terms, every[k] if eq is not None else None)
        r = challenge(g)
        rounds.append(g)
        point.append(r)
        every = [M.fix_variables(F, T, [r]) for T in every]
    return (rounds[0][0] + rounds[0][1]) % F.p, rounds, point, [T[0] for T in every]


def verify(F, terms, has_eq, claimed_sum, rounds, point, final_evals):
    """every round interpolated at 0 .. D: g_i(0) + g_i(1) is the running claim (the claimed sum first), and at the end
    E(point) * sum_t c_t prod T_m(point) = g_n(r_n)"""
    p = F.p
    if len(rounds) != len(point) or not rounds:
        return False
    D = degree(terms, has_eq)
    expect = F.plain(claimed_sum)
    for g, r in zip(rounds, point):
        if len(g) != D + 1:
            return False
        ys = [F.plain(v) for v in g]
        if (ys[0] + ys[1]) % p != expect:
            return False
        expect = M.interpolate(p, ys, F.plain(r))
    tabs = final_evals[:-1] if has_eq else final_evals
    b = bracket(F, terms, tabs)
    last = F.mul(final_evals[-1], b) if has_eq else b
    return F.plain(last) == expect


def term_lists(F, M, coeffs):
    """The term lists the tests run over M tables A, B, C, D = 0, 1, 2, 3; coeffs: at least three general coefficients.
      A B - C                      M >= 3, the coefficient minus one
      rA A D + rB B D + rC C D     M = 4, general coefficients
      A B C + D                    M = 4
      all                          one term over every table (over A, B, C when M = 4: a term takes at most three)
      eight                        eight terms over the subsets of at most three tables in turn, with the coefficients
                                   None, general, minus one, one, zero in turn"""
    import itertools
    minus_one = F.elem(F.p - 1)
    lists = {}
    if M >= 3:
        lists["A B - C"] = [(None, (0, 1)), (minus_one, (2,))]
    if M == 4:
        lists["rA A D + rB B D + rC C D"] = [(coeffs[0], (0, 3)), (coeffs[1], (1, 3)), (coeffs[2], (2, 3))]
        lists["A B C + D"] = [(None, (0, 1, 2)), (None, (3,))]
    lists["all"] = [(None, tuple(range(min(M, 3))))]
    subsets = [s for size in (1, 2, 3) for s in itertools.combinations(range(M), size)]
    cs = [None, coeffs[0], minus_one, F.one, 0, coeffs[1], None, coeffs[2]]
    lists["eight"] = [(cs[t], subsets[(5 * t + 1) % len(subsets)]) for t in range(8)]
    return lists


def eq_closed_form(F, r, s):
    """eq(r, s) = prod_j (r_j s_j + (1 - r_j)(1 - s_j)) as an element"""
    acc = F.one
    for a, b in zip(r, s):
        f = (F.mul(a, b) + F.mul((F.one - a) % F.p, (F.one - b) % F.p)) % F.p
        acc = F.mul(acc, f)
    return acc
