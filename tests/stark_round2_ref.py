"""Python big-integer restatement of the STARK prover's round 2 for the tests of stark_round2.hip:
ConstraintEvaluator::evaluate (provers/stark/src/constraints/evaluator.rs:33-225) with Frame::read_from_lde's row
arithmetic, zerofier_evaluations_on_extended_domain and end_exemptions_poly (constraints/transition.rs:88-205) with all
their branches and truncating integer divisions, break_in_parts (math/src/polynomial/mod.rs:289-302) and
commit_composition_polynomial (provers/stark/src/prover.rs:398-425).  Values are canonical integers; the transforms of the
larger shapes go through the oracle's NTT."""
import numpy as np

from oracle import bigint_def as D
from oracle import oracle as O

R = 1 << 256


def to_stored(p, vals):
    """canonical integers -> (n, 4) uint64 in the reference's memory form (Montgomery, MS limb first)"""
    return O.ints_to_array([v * R % p for v in vals], 4)


def from_stored(p, arr):
    rinv = pow(R, -1, p)
    return [v * rinv % p for v in O.array_to_ints(np.asarray(arr).reshape(-1, 4))]


def stored_one(p, v):
    return to_stored(p, [v])[0]


class Domain:
    """provers/stark/src/domain.rs: trace length n, blow-up, coset offset h (canonical)"""

    def __init__(self, p, log2_trace, log2_blowup, offset):
        self.p, self.n, self.blowup, self.h = p, 1 << log2_trace, 1 << log2_blowup, offset % p
        self.N = self.n * self.blowup
        self.log2_lde = log2_trace + log2_blowup
        self.g = D.primitive_root_of_unity(p, log2_trace)        # trace_primitive_root
        self.w = D.primitive_root_of_unity(p, self.log2_lde)    # lde root
        self._coset = None

    @property
    def coset(self):
        """lde_roots_of_unity_coset: x_i = h w^i"""
        if self._coset is None:
            x, out = self.h, []
            for _ in range(self.N):
                out.append(x)
                x = x * self.w % self.p
            self._coset = out
        return self._coset


def frame_row(dom, i, offset):
    """Frame::read_from_lde (provers/stark/src/frame.rs): the LDE row of trace step `offset` ahead of LDE row i"""
    return (i + offset * dom.blowup) % dom.N


def end_exemptions_roots(dom, t):
    return [pow(dom.g, dom.n - k * t["period"], dom.p) for k in range(1, t.get("end_exemptions", 0) + 1)]


def end_exemptions_evaluations(dom, t):
    """end_exemptions_poly evaluated on the LDE coset (the reference runs an LDE of it; the values are the same)"""
    p, roots = dom.p, end_exemptions_roots(dom, t)
    out = []
    for x in dom.coset:
        e = 1
        for r in roots:
            e = e * (x - r) % p
        out.append(e)
    return out


def zerofier_evaluations_on_extended_domain(dom, t):
    """constraints/transition.rs:108-205, both branches"""
    p, n, g = dom.p, dom.n, dom.g
    period, offset = t.get("period", 1), t.get("offset", 0)
    ep = t.get("exemptions_period") or 0
    den_const = pow(g, offset * n // period, p)
    if ep:
        num_const = pow(g, n * (t.get("periodic_exemptions_offset") or 0) // ep, p)
        cycle = []
        for e in range(min(dom.blowup * ep, dom.N)):
            x = dom.h * pow(dom.w, e, p) % p
            num = (pow(x, n // ep, p) - num_const) % p
            den = (pow(x, n // period, p) - den_const) % p
            cycle.append(num * pow(den, -1, p) % p)
    else:
        cycle = []
        for e in range(min(dom.blowup * period, dom.N)):
            x = dom.h * pow(dom.w, e, p) % p
            cycle.append(pow((pow(x, n // period, p) - den_const) % p, -1, p))
    ee = end_exemptions_evaluations(dom, t)
    return [cycle[i % len(cycle)] * ee[i] % p for i in range(dom.N)]


def evaluate(dom, columns, boundary, transitions, transition_evals):
    """ConstraintEvaluator::evaluate.  columns: canonical LDE columns (main, then auxiliary); boundary: [(col, step, value,
    coeff)]; transitions: [dict(period, offset, end_exemptions, exemptions_period, periodic_exemptions_offset, coeff)];
    transition_evals[c][i]: compute_transition's value of constraint c at LDE row i."""
    p = dom.p
    out = [0] * dom.N
    for col, step, value, coeff in boundary:
        point = pow(dom.g, step, p)
        for i, x in enumerate(dom.coset):
            out[i] = (out[i] + pow((x - point) % p, -1, p) * coeff % p * ((columns[col][i] - value) % p)) % p
    for c, t in enumerate(transitions):
        z = zerofier_evaluations_on_extended_domain(dom, t)
        for i in range(dom.N):
            out[i] = (out[i] + z[i] * transition_evals[c][i] % p * t["coeff"]) % p
    return out


def break_in_parts(coeffs, n_parts):
    """-> (blocks zero padded to L = next_power_of_two(ceil(N / P)), stripped lengths)"""
    per = -(-len(coeffs) // n_parts)
    L = 1 << (per - 1).bit_length()
    blocks, lens = [], []
    for j in range(n_parts):
        c = list(coeffs[j::n_parts])
        ln = len(c)
        while ln and c[ln - 1] == 0:
            ln -= 1
        blocks.append(c + [0] * (L - len(c)))
        lens.append(ln)
    return blocks, lens


def evaluate_on_coset(dom, coeffs):
    """values at x_0 .. x_{N-1} by Horner's rule (small shapes)"""
    out = []
    for x in dom.coset:
        acc = 0
        for c in reversed(coeffs):
            acc = (acc * x + c) % dom.p
        out.append(acc)
    return out


def composition_nodes(parts_lde_stored):
    """commit_composition_polynomial: (P, N, 4) stored LDE of the parts -> nodes (N - 1, 32), root first: the tree over the
    2 P half-columns [p_0 lo, .., p_{P-1} lo, p_0 hi, ..] of N / 2 rows, bit-reverse permuted"""
    a = np.ascontiguousarray(parts_lde_stored, dtype=np.uint64)
    half = a.shape[1] // 2
    return O.merkle_commit_columns(np.concatenate([a[:, :half], a[:, half:]]), bit_reverse=True)


def composition_nodes_by_rows(parts_lde_stored):
    """the same tree built the way the reference writes it: rows, in_place_bit_reverse_permute, chunks(2) merged, one
    Keccak per leaf, parents of pairs (small shapes)"""
    a = np.ascontiguousarray(parts_lde_stored, dtype=np.uint64)
    n_rows = a.shape[1]
    bits = n_rows.bit_length() - 1
    rows = [b"".join(int(w).to_bytes(8, "big") for w in a[:, D.bit_reverse(j, bits)].reshape(-1)) for j in range(n_rows)]
    level = [O.keccak256(rows[2 * i] + rows[2 * i + 1]) for i in range(n_rows // 2)]
    levels = [level]
    while len(level) > 1:
        level = [O.keccak256(level[2 * i] + level[2 * i + 1]) for i in range(len(level) // 2)]
        levels.append(level)
    flat = [h for lv in reversed(levels) for h in lv]
    return np.frombuffer(b"".join(flat), np.uint8).reshape(-1, 32)


def fibonacci_2_cols_shifted_case(golden):
    """Stone-compatibility case 1 (provers/stark/src/prover.rs:1208-1360) from tests/golden/stark_round2.json: the trace
    columns, the constraint tables and the transition evaluations on the LDE, all canonical."""
    from tests import util
    p = D.P_STARK252
    dom = Domain(p, golden["log2_trace"], golden["log2_blowup"], golden["coset_offset"])
    c0, c1 = util.stone_compat_trace_columns(int(golden["trace_initial"], 16), dom.n)
    lde = []
    for col in (c0, c1):
        coeffs = D.interpolate_fft_def(col, p)
        lde.append(evaluate_on_coset(dom, coeffs))
    beta = int(golden["beta"], 16)
    transitions = [dict(period=1, offset=0, end_exemptions=1, coeff=1), dict(period=1, offset=0, end_exemptions=1, coeff=beta)]
    boundary = [(0, 0, 1, pow(beta, 2, p)), (0, 3, 3, pow(beta, 3, p))]
    t0 = [(lde[0][frame_row(dom, i, 1)] - lde[1][i]) % p for i in range(dom.N)]
    t1 = [(lde[1][frame_row(dom, i, 1)] - lde[0][i] - lde[1][i]) % p for i in range(dom.N)]
    return dom, lde, boundary, transitions, [t0, t1]


def stored_tables(p, boundary, transitions):
    """canonical tables -> the stored-form tables stark.constraint_evaluations_device takes"""
    b = [(col, step, stored_one(p, value), stored_one(p, coeff)) for col, step, value, coeff in boundary]
    t = [dict(tr, coeff=stored_one(p, tr["coeff"])) for tr in transitions]
    return b, t
