"""Python big-integer model of the randomized AIR over a small field F with its extension E (csrc/ext_aux.cuh and the _rap_
part of csrc/ext_round2.cuh, csrc/air_program.h): the auxiliary column as a running product or sum of fractions, the typing
of an AIR program whose operands are words of F or elements of E, the program run at one LDE row, the evaluations of the
composition polynomial and its value at an out-of-domain point.  Fields, domains and words are those of ext_round2_ref;
a value of F is an int, an element of E a tuple."""
from tests import air_program_ref as A
from tests import ext_round2_ref as M
from tests import stark_round2_ref as R2

XCELL, XCONST = 3, 4
PRODUCT, SUM = 0, 1
TYPED_ACC_EXT, TYPED_SRC_EXT = 1 << 4, 1 << 5


def one(F):
    return M.lift(F, 1)


# ---- the auxiliary column
def fractions(F, cols, n, num, den):
    """num = (a_0, [(col, a_j)]), den likewise, the scalars in E -> ([numerator_i], [denominator_i]) for i < n"""
    E = F.ext

    def side(s, i):
        v = s[0]
        for col, coeff in s[1]:
            v = E.add(v, E.mul_base(coeff, cols[col][i] % F.p))
        return v

    return [side(num, i) for i in range(n)], [side(den, i) for i in range(n)]


def fraction_values(F, cols, n, num, den):
    """-> ([f_i], the number of zero denominators); a fraction with a zero denominator counts as zero"""
    E = F.ext
    nums, dens = fractions(F, cols, n, num, den)
    return [E.mul(a, E.inv(b)) if b != F.zero else F.zero for a, b in zip(nums, dens)], sum(1 for d in dens if d == F.zero)


def running(F, values, mode, exclusive):
    """-> (the running product or sum of the values, inclusive or exclusive; the product or sum of all)"""
    E = F.ext
    run = one(F) if mode == PRODUCT else F.zero
    out = []
    for f in values:
        if exclusive:
            out.append(run)
        run = E.mul(run, f) if mode == PRODUCT else E.add(run, f)
        if not exclusive:
            out.append(run)
    return out, run


def aux_fractions(F, cols, n, num, den, mode, exclusive):
    """-> (the n elements of the column, the product or sum over all rows, the number of zero denominators)"""
    values, zeros = fraction_values(F, cols, n, num, den)
    out, total = running(F, values, mode, exclusive)
    return out, total, zeros


def rom_aux_column(F, a, v, a_sorted, v_sorted, z, alpha):
    """read_only_memory.rs:281-310 restated: aux[0] = (z - (a_0 + alpha v_0)) / (z - (as_0 + alpha vs_0)), then
    aux[i] = aux[i-1] (z - (a_i + alpha v_i)) / (z - (as_i + alpha vs_i))"""
    E = F.ext
    term = lambda x, y: E.sub(z, E.add(M.lift(F, x), E.mul_base(alpha, y)))
    out = []
    for i in range(len(a)):
        f = E.mul(term(a[i], v[i]), E.inv(term(a_sorted[i], v_sorted[i])))
        out.append(f if i == 0 else E.mul(out[-1], f))
    return out


def fib_rap_aux_column(F, not_perm, perm, gamma):
    """fibonacci_rap.rs:205-233 restated: aux[0] = 1, aux[i+1] = aux[i] (not_perm[i] + gamma) / (perm[i] + gamma) for
    i < n - 1"""
    E = F.ext
    out = [one(F)]
    for i in range(len(not_perm) - 1):
        f = E.mul(E.add(M.lift(F, not_perm[i]), gamma), E.inv(E.add(M.lift(F, perm[i]), gamma)))
        out.append(E.mul(out[-1], f))
    return out


# ---- the typing of a program
def type_program(ops, degree):
    """ops: [(op, src, index, row)] -> (the typed op words the kernel reads, n_tmps, the number of temporaries that hold an
    element of E at some point, LDS slots per lane).  The model of air_program_check_rap."""
    acc_ext, tmp_ext, ever = False, {}, set()
    bits = []
    for op, src, index, row in ops:
        if op <= A.MUL:
            src_ext = src in (XCELL, XCONST) or (src == A.TMP and tmp_ext[index])
            bits.append((TYPED_ACC_EXT if op != A.LOAD and acc_ext else 0) | (TYPED_SRC_EXT if src_ext else 0))
            acc_ext = src_ext if op == A.LOAD else acc_ext or src_ext
        else:
            bits.append(TYPED_ACC_EXT if acc_ext else 0)
            if op == A.STORE:
                tmp_ext[index] = acc_ext
                if acc_ext:
                    ever.add(index)
    n_tmps = max(tmp_ext) + 1 if tmp_ext else 0
    base, slots = {}, 0
    for t in range(n_tmps):
        base[t] = slots
        slots += degree if t in ever else 1
    words = []
    for (op, src, index, row), b in zip(ops, bits):
        if op == A.STORE or (op <= A.MUL and src == A.TMP):
            index = base[index]
        words.append(op | b | src << 8 | index << 16 | row << 32)
    return words, n_tmps, len(ever), slots


# ---- the program at one row
class Arith:
    """+, -, * on values that are ints (F) or tuples (E); the result is in E as soon as one operand is"""

    def __init__(self, F):
        self.F, self.E, self.p = F, F.ext, F.p

    def lift(self, v):
        return v if isinstance(v, tuple) else M.lift(self.F, v)

    def add(self, a, b):
        if isinstance(a, tuple) or isinstance(b, tuple):
            return self.E.add(self.lift(a), self.lift(b))
        return (a + b) % self.p

    def sub(self, a, b):
        if isinstance(a, tuple) or isinstance(b, tuple):
            return self.E.sub(self.lift(a), self.lift(b))
        return (a - b) % self.p

    def mul(self, a, b):
        if isinstance(a, tuple) and isinstance(b, tuple):
            return self.E.mul(a, b)
        if isinstance(a, tuple):
            return self.E.mul_base(a, b)
        if isinstance(b, tuple):
            return self.E.mul_base(b, a)
        return a * b % self.p

    def neg(self, a):
        return self.sub(0, a) if not isinstance(a, tuple) else self.E.sub(self.F.zero, a)


def run(F, ops, source, ar=None):
    """the op list with source(src, index, row) giving the operands -> {constraint: value (an int or a tuple)}"""
    ar = ar or Arith(F)
    acc, tmp, out = None, {}, {}
    for op, src, index, row in ops:
        if op <= A.MUL:
            s = tmp[index] if src == A.TMP else source(src, index, row)
            acc = s if op == A.LOAD else ar.add(acc, s) if op == A.ADD else ar.sub(acc, s) if op == A.SUB else ar.mul(acc, s)
        elif op == A.NEG:
            acc = ar.neg(acc)
        elif op == A.STORE:
            tmp[index] = acc
        else:
            out[index] = acc
    return out


def evaluate(F, dom, cols, aux, ops, consts, xconsts, boundary, transitions):
    """out[i] = sum_c coeff_c Z_c[i] T_c(i) + sum_k coeff_k (col_k[i] - value_k) / (x_i - g^step_k): cols canonical LDE columns
    of F, aux LDE columns of E (lists of tuples), boundary [(col, step, value (int or tuple), coeff, is_aux)]"""
    p, E, ar = F.p, F.ext, Arith(F)
    ops = [tuple(int(x) for x in o) for o in ops]
    out = [F.zero] * dom.N
    for col, step, value, coeff, is_aux in boundary:
        point = pow(dom.g, step, p)
        for i, x in enumerate(dom.coset):
            num = E.sub(ar.lift(aux[col][i] if is_aux else cols[col][i]), ar.lift(value))
            out[i] = E.add(out[i], E.mul(coeff, E.mul_base(num, pow((x - point) % p, -1, p))))
    zs = {}
    for t in transitions:
        key = tuple(t.get(k) or 0 for k in ("period", "offset", "end_exemptions", "exemptions_period", "periodic_exemptions_offset"))
        if key not in zs:
            zs[key] = R2.zerofier_evaluations_on_extended_domain(dom, t)
    for i in range(dom.N if transitions else 0):
        def source(src, index, row):
            if src == A.CELL:
                return A.read_cell(dom, cols, index, row, i)
            if src == XCELL:
                return aux[index][R2.frame_row(dom, i, row) % dom.N]
            return consts[index] if src == A.CONST else xconsts[index]
        T = run(F, ops, source, ar)
        for c, t in enumerate(transitions):
            key = tuple(t.get(k) or 0 for k in ("period", "offset", "end_exemptions", "exemptions_period", "periodic_exemptions_offset"))
            out[i] = E.add(out[i], E.mul(t["coeff"], E.mul_base(ar.lift(T[c]), zs[key][i])))
    return out


def composition_at(F, dom, trace_polys, aux_polys, ops, consts, xconsts, boundary, transitions, z):
    """sum_c coeff_c T_c(z) Z_c(z) + boundary(z) in E at z outside F.  trace_polys: coefficient lists in F; aux_polys:
    coefficient lists in E (tuples)"""
    E, p, ar = F.ext, F.p, Arith(F)
    ops = [tuple(int(x) for x in o) for o in ops]
    memo = {}

    def source(src, index, row):
        if src in (A.CELL, XCELL):
            if (src, index, row) not in memo:
                poly = [M.lift(F, c) for c in trace_polys[index]] if src == A.CELL else aux_polys[index]
                memo[(src, index, row)] = M.horner_ext(F, poly, E.mul_base(z, pow(dom.g, row, p)))
            return memo[(src, index, row)]
        return consts[index] if src == A.CONST else xconsts[index]

    T = run(F, ops, source, ar)
    total = F.zero
    for c, t in enumerate(transitions):
        period, n = t.get("period", 1), dom.n
        zf = E.inv(E.sub(E.power(z, n // period), M.lift(F, pow(dom.g, t.get("offset", 0) * n // period, p))))
        for r in R2.end_exemptions_roots(dom, t):
            zf = E.mul(zf, E.sub(z, M.lift(F, r)))
        total = E.add(total, E.mul(t["coeff"], E.mul(ar.lift(T[c]), zf)))
    for col, step, value, coeff, is_aux in boundary:
        q = E.mul(E.sub(source(XCELL if is_aux else A.CELL, col, 0), ar.lift(value)), E.inv(E.sub(z, M.lift(F, pow(dom.g, step, p)))))
        total = E.add(total, E.mul(coeff, q))
    return total


# ---- the two example AIRs with their z column as an auxiliary column and the challenges in E
def rom_rap(S):          # read_only_memory.rs; columns a, v, a_sorted, v_sorted; aux p; constant 1; extension constants z, alpha
    one_, z, alpha = S.const(0), S.xconst(0), S.xconst(1)
    step = S.cell(2, 1) - S.cell(2) - one_
    return [(S.cell(2, 1) - S.cell(2)) * step,
            (S.cell(3, 1) - S.cell(3)) * step,
            (z - (alpha * S.cell(3, 1) + S.cell(2, 1))) * S.xcell(0, 1) - (z - (alpha * S.cell(1, 1) + S.cell(0, 1))) * S.xcell(0)]


def fib_rap_rap(S):      # fibonacci_rap.rs; columns a, b; aux z; extension constant gamma
    gamma = S.xconst(0)
    return [S.xcell(0, 1) * (gamma + S.cell(1)) - S.xcell(0) * (gamma + S.cell(0))]


RAP_AIRS = {"rom": (rom_rap, 4, 1, 2), "fib_rap": (fib_rap_rap, 2, 0, 1)}   # builder, main columns, constants, extension constants
