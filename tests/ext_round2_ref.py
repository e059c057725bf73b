"""Python big-integer model of STARK round 2 over a small field F with its extension E (csrc/ext_round2.cuh): the
evaluations of the composition polynomial on the LDE coset, with the AIR's program run by air_program_ref, the zerofiers
and break_in_parts of stark_round2_ref (both take p as an argument) and the extension arithmetic of goldilocks_ext_ref
(Fp2 over Goldilocks) and babybear_ext_ref (Fp4 over BabyBear).  Values are canonical integers, an element of E a tuple of
them; WORD / UNWORD go between a canonical value and the word the library stores (the value itself for Goldilocks, the
Montgomery value for BabyBear)."""
from tests import air_program_ref as A
from tests import babybear_ext_ref as B
from tests import goldilocks_ext_ref as X
from tests import goldilocks_ref as G
from tests import stark_round2_ref as R2


class Field:
    def __init__(self, name, p, width, ext, root, word, unword):
        self.name, self.p, self.width, self.ext, self.root, self.word, self.unword = name, p, width, ext, root, word, unword
        self.zero = (0,) * width

    def word_elem(self, a):
        return tuple(self.word(c) for c in a)

    def unword_elem(self, a):
        return tuple(self.unword(int(c)) for c in a)


GL2 = Field("gl2", G.P, 2, X, G.root_of_unity, lambda v: int(v) % G.P, lambda w: G.reduce_word(int(w)))   # Goldilocks has no entry in FFT_PARAMS
BB4 = Field("bb4", B.P, 4, B, B.root_of_unity, B.store, B.unstore)
FIELDS = {"gl2": GL2, "bb4": BB4}


def domain(F, log2_trace, log2_blowup, offset):
    """stark_round2_ref.Domain with the library's roots of F (offset canonical)"""
    d = R2.Domain.__new__(R2.Domain)
    d.p, d.n, d.blowup, d.h = F.p, 1 << log2_trace, 1 << log2_blowup, offset % F.p
    d.N = d.n * d.blowup
    d.log2_lde = log2_trace + log2_blowup
    d.g, d.w = F.root(log2_trace), F.root(d.log2_lde)
    d._coset = None
    return d


def evaluate(F, dom, cols, ops, consts, boundary, transitions):
    """out[i] = sum_c coeff_c Z_c[i] T_c(i) + sum_k coeff_k (col_k[i] - value_k) / (x_i - g^step_k): cols canonical LDE
    columns (a periodic one short), ops the program, consts canonical, boundary [(col, step, value, coeff in E)],
    transitions [dict(..., coeff in E)] -> N elements of E"""
    p, E = F.p, F.ext
    out = [F.zero] * dom.N
    for col, step, value, coeff in boundary:
        point = pow(dom.g, step, p)
        for i, x in enumerate(dom.coset):
            out[i] = E.add(out[i], E.mul_base(coeff, pow((x - point) % p, -1, p) * ((cols[col][i] - value) % p) % p))
    if transitions:
        T = A.run_all(ops, dom, cols, consts, len(transitions))
        zs = {}
        for c, t in enumerate(transitions):
            key = tuple(t.get(k) or 0 for k in ("period", "offset", "end_exemptions", "exemptions_period", "periodic_exemptions_offset"))
            if key not in zs:
                zs[key] = R2.zerofier_evaluations_on_extended_domain(dom, t)
            z = zs[key]
            for i in range(dom.N):
                out[i] = E.add(out[i], E.mul_base(t["coeff"], z[i] * T[c][i] % p))
    return out


def interpolate(dom, evals):
    """interpolate_offset_fft by definition: the N coefficients of the polynomial with value evals[i] at h w^i"""
    p, N = dom.p, dom.N
    winv, hinv, ninv = pow(dom.w, -1, p), pow(dom.h, -1, p), pow(N, -1, p)
    wp = [pow(winv, k, p) for k in range(N)]
    out, hj = [], ninv
    for j in range(N):
        out.append(sum(evals[i] * wp[i * j % N] for i in range(N)) % p * hj % p)
        hj = hj * hinv % p
    return out


def parts(F, dom, evals, n_parts):
    """evals: N elements of E -> (coefficient planes [P D][L], stripped lengths [P], LDE planes [P D][N]); part j, plane e
    at index j D + e; the length of a part is the last index where any plane is not zero, plus one"""
    H = [interpolate(dom, [v[e] for v in evals]) for e in range(F.width)]
    blocks = [R2.break_in_parts(H[e], n_parts) for e in range(F.width)]
    coeffs = [blocks[e][0][j] for j in range(n_parts) for e in range(F.width)]
    lens = [max(blocks[e][1][j] for e in range(F.width)) for j in range(n_parts)]
    return coeffs, lens, [R2.evaluate_on_coset(dom, c) for c in coeffs]


def horner_ext(F, coeffs, z):
    """sum_i coeffs[i] z^i for coefficients in E and z in E"""
    acc = F.zero
    for c in reversed(coeffs):
        acc = F.ext.add(F.ext.mul(acc, z), c)
    return acc


def lift(F, v):
    return (v % F.p,) + (0,) * (F.width - 1)


def composition_at(F, dom, trace_polys, ops, consts, boundary, transitions, z):
    """sum_c coeff_c T_c(z) Z_c(z) + boundary(z) in E for z outside F: the program runs on the trace polynomials'
    values at z g^row, all arithmetic in E"""
    E, p = F.ext, F.p
    zg = {}

    def cell(col, row):
        if (col, row) not in zg:
            zg[(col, row)] = horner_ext(F, [lift(F, c) for c in trace_polys[col]], E.mul_base(z, pow(dom.g, row, p)))
        return zg[(col, row)]

    acc, tmp, T = None, {}, {}
    for op, src, index, row in ops:
        op, src, index, row = int(op), int(src), int(index), int(row)
        if op <= A.MUL:
            s = cell(index, row) if src == A.CELL else lift(F, consts[index]) if src == A.CONST else tmp[index]
            acc = s if op == A.LOAD else E.add(acc, s) if op == A.ADD else E.sub(acc, s) if op == A.SUB else E.mul(acc, s)
        elif op == A.NEG:
            acc = E.sub(F.zero, acc)
        elif op == A.STORE:
            tmp[index] = acc
        else:
            T[index] = acc
    total = F.zero
    for c, t in enumerate(transitions):
        period, n = t.get("period", 1), dom.n
        den = E.sub(E.power(z, n // period), lift(F, pow(dom.g, t.get("offset", 0) * n // period, p)))
        zf = E.inv(den)
        ep = t.get("exemptions_period") or 0
        if ep:
            zf = E.mul(zf, E.sub(E.power(z, n // ep), lift(F, pow(dom.g, n * (t.get("periodic_exemptions_offset") or 0) // ep, p))))
        for r in R2.end_exemptions_roots(dom, t):
            zf = E.mul(zf, E.sub(z, lift(F, r)))
        total = E.add(total, E.mul(t["coeff"], E.mul(T[c], zf)))
    for col, step, value, coeff in boundary:
        q = E.mul(E.sub(cell(col, 0), lift(F, value)), E.inv(E.sub(z, lift(F, pow(dom.g, step, p)))))
        total = E.add(total, E.mul(coeff, q))
    return total
