"""Circle STARK round 2 over Mersenne31 with QM31 in plain integers, the yardstick of csrc/circle_round2.cuh, on top of
circle_ref (the circle group, the transforms), mersenne31_ext_ref (QM31) and air_program_ref (the interpreter):

    out[i] = sum_c beta_c T_c(i) E_c(q_i) / Z_c(q_i)  +  sum_k gamma_k (col_k[i] - v_k) (1 + x'_k) / y'_k

on the LDE coset q_i = g_2N + i g_N, with the trace points p_j = g_2n + j g_n.  The same formulas over QM31 give the
prover's identity at an out-of-domain point of the circle.  Values are canonical integers; an element of QM31 is a tuple."""
from tests import air_program_ref as A
from tests import circle_ref as CR
from tests import mersenne31_ext_ref as R

P = CR.P


class Domain:
    """trace 2^log2_trace, blow-up 2^log2_blowup: the fields air_program_ref reads (p, blowup, N) and the two point sets"""

    def __init__(self, log2_trace, log2_blowup):
        self.p, self.log2_trace, self.log2_blowup, self.log2_lde = P, log2_trace, log2_blowup, log2_trace + log2_blowup
        self.n, self.blowup = 1 << log2_trace, 1 << log2_blowup
        self.N = self.n * self.blowup
        self.trace_points = CR.coset_points(log2_trace)
        self.lde_points = CR.coset_points(self.log2_lde)


def psub(a, c):
    """A - C in the circle group"""
    return ((a[0] * c[0] + a[1] * c[1]) % P, (a[1] * c[0] - a[0] * c[1]) % P)


def log2(m):
    assert m >= 1 and m & (m - 1) == 0
    return m.bit_length() - 1


# ---- the zerofier and the exemptions at a point of the circle over F_p
def zerofier(dom, t, Q):
    """Z(Q) = y(2^(mu-1) (Q - p_offset)), m = n / period = 2^mu"""
    d = psub(Q, dom.trace_points[t.get("offset", 0)])
    for _ in range(log2(dom.n // t.get("period", 1)) - 1):
        d = CR.pdouble(d)
    return d[1]


def exemption_points(dom, t):
    period, offset, m = t.get("period", 1), t.get("offset", 0), dom.n // t.get("period", 1)
    return [dom.trace_points[offset + (m - k) * period] for k in range(1, t.get("end_exemptions", 0) + 1)]


def exemptions(dom, t, Q):
    """E(Q) = prod_k (1 - x(Q - P_k))"""
    e = 1
    for pk in exemption_points(dom, t):
        e = e * (1 - (pk[0] * Q[0] + pk[1] * Q[1])) % P
    return e


def boundary_factor(dom, step, Q):
    """(1 + x') / y', (x', y') = Q - p_step"""
    x, y = psub(Q, dom.trace_points[step])
    return (1 + x) * CR.inv(y) % P


def constrained_rows(dom, t):
    """the trace rows where the quotient T E / Z asks T to vanish"""
    period, offset = t.get("period", 1), t.get("offset", 0)
    rows = list(range(offset, dom.n, period))
    return rows[: len(rows) - t.get("end_exemptions", 0)]


# ---- the evaluations on the LDE coset
def evaluate(dom, cols, ops, consts, boundary, transitions):
    """cols: canonical columns (a short one wraps at its own length); boundary: [(col, step, value, gamma)]; transitions:
    [dict(period, offset, end_exemptions, coeff)] -> N elements of QM31"""
    ops = [tuple(int(x) for x in o) for o in ops]
    table = {}
    for t in transitions:
        key = (t.get("period", 1), t.get("offset", 0), t.get("end_exemptions", 0))
        if key not in table:
            table[key] = [exemptions(dom, t, q) * CR.inv(zerofier(dom, t, q)) % P for q in dom.lde_points]
    out = []
    for i, q in enumerate(dom.lde_points):
        total = R.ZERO
        emitted = A.run(ops, dom, cols, consts, i) if transitions else {}
        for c, t in enumerate(transitions):
            key = (t.get("period", 1), t.get("offset", 0), t.get("end_exemptions", 0))
            total = R.add(total, R.mul_base(t["coeff"], emitted[c] * table[key][i] % P))
        for col, step, value, gamma in boundary:
            total = R.add(total, R.mul_base(gamma, (cols[col][i] - value) * boundary_factor(dom, step, q) % P))
        out.append(total)
    return out


# ---- the parts
def interpolate(evals):
    """N elements -> the four planes of N coefficients"""
    return [CR.interpolate_cfft([v[e] for v in evals]) for e in range(4)]


def parts(dom, evals, log2_part, n_parts):
    """-> (4 P planes of L coefficients, 4 P planes of N values on the LDE coset, the non-zero words from P L on); part j,
    plane e at 4 j + e"""
    L = 1 << log2_part
    H = interpolate(evals)
    coeffs = [H[e][j * L:(j + 1) * L] for j in range(n_parts) for e in range(4)]
    lde = [CR.evaluate_cfft(c + [0] * (dom.N - L)) for c in coeffs]
    tail = sum(1 for e in range(4) for w in H[e][n_parts * L:] if w)
    return coeffs, lde, tail


def pi_iter(x, k):
    """pi^k(x) over QM31, pi(x) = 2 x^2 - 1"""
    for _ in range(k):
        x = R.sub(R.mul_base(R.sqr(x), 2), R.ONE)
    return x


def part_factors(point, log2_part, n_parts):
    """M_j = prod_{t: bit t of j set} pi^(log2_part + t - 1)(X)"""
    out = []
    for j in range(n_parts):
        m = R.ONE
        for t in range(j.bit_length()):
            if (j >> t) & 1:
                m = R.mul(m, pi_iter(point[0], log2_part + t - 1))
        out.append(m)
    return out


def last_nonzero(evals):
    """the highest coefficient index where a plane of the interpolated evaluations is not zero (-1: none)"""
    H = interpolate(evals)
    return max([k for e in range(4) for k, w in enumerate(H[e]) if w], default=-1)


def degree_bound(dom, degree, end_exemptions, period=1):
    """the statement of lw_hip.h: total degree D <= d n / 2 + 2 e - m / 2 (and n / 2 for a boundary constraint); no coefficient
    at or above the smallest power of two greater than 2 D"""
    D = max(degree * dom.n // 2 + 2 * end_exemptions - dom.n // period // 2, dom.n // 2)
    b = 1
    while b <= 2 * D:
        b *= 2
    return b


# ---- the same formulas at a point of the circle over QM31: the prover's identity
def q_padd(a, b):
    return R.sub(R.mul(a[0], b[0]), R.mul(a[1], b[1])), R.add(R.mul(a[0], b[1]), R.mul(a[1], b[0]))


def q_psub(a, c):
    return R.add(R.mul(a[0], c[0]), R.mul(a[1], c[1])), R.sub(R.mul(a[1], c[0]), R.mul(a[0], c[1]))


def q_pdouble(a):
    return R.sub(R.mul_base(R.sqr(a[0]), 2), R.ONE), R.mul_base(R.mul(a[0], a[1]), 2)


def lift(pt):
    return R.embed(pt[0]), R.embed(pt[1])


def frame_points(dom, z, rows):
    """z + r g_n for the trace-row offsets r"""
    g = CR.subgroup_generator(dom.log2_trace)
    return [q_padd(z, lift(CR.pmul(r, g))) if r else z for r in rows]


def periodic_point(dom, period, pt):
    """(n / period) pt: where the period's own polynomial of `period` coefficients is read"""
    for _ in range(log2(dom.n // period)):
        pt = q_pdouble(pt)
    return pt


def composition_at(dom, cell, ops, consts, boundary, transitions, z):
    """sum_c beta_c T_c E_c / Z_c + sum_k gamma_k (t_k(z) - v_k)(1 + x') / y' at z, a point of the circle over QM31.
    cell(col, row) -> the value of column col at z + row g_n, an element of QM31."""
    acc, tmp, emitted = None, [None] * A.MAX_TMPS, {}
    for op, src, index, row in [tuple(int(x) for x in o) for o in ops]:
        if op <= A.MUL:
            s = cell(index, row) if src == A.CELL else R.embed(consts[index]) if src == A.CONST else tmp[index]
            acc = s if op == A.LOAD else R.add(acc, s) if op == A.ADD else R.sub(acc, s) if op == A.SUB else R.mul(acc, s)
        elif op == A.NEG:
            acc = R.neg(acc)
        elif op == A.STORE:
            tmp[index] = acc
        else:
            emitted[index] = acc
    total = R.ZERO
    for c, t in enumerate(transitions):
        d = q_psub(z, lift(dom.trace_points[t.get("offset", 0)]))
        for _ in range(log2(dom.n // t.get("period", 1)) - 1):
            d = q_pdouble(d)
        e = R.ONE
        for pk in exemption_points(dom, t):
            e = R.mul(e, R.sub(R.ONE, R.add(R.mul_base(z[0], pk[0]), R.mul_base(z[1], pk[1]))))
        total = R.add(total, R.mul(t["coeff"], R.mul(emitted[c], R.mul(e, R.inv(d[1])))))
    for col, step, value, gamma in boundary:
        x, y = q_psub(z, lift(dom.trace_points[step]))
        total = R.add(total, R.mul(gamma, R.mul(R.sub(cell(col, 0), R.embed(value)), R.mul(R.add(R.ONE, x), R.inv(y)))))
    return total
