"""Python big-integer reference of the AIR transition programs of csrc/stark_air.hip: the interpreter of an op list
(lw_stark_air_op_t, include/lw_hip.h) at one LDE row, the direct evaluation of an expression tree, and the reference's
example AIRs (provers/stark/src/examples/*.rs) written as expressions.  Values are canonical integers; cells are read with
stark_round2_ref.frame_row (Frame::read_from_lde)."""
import numpy as np

from tests import stark_round2_ref as R2

LOAD, ADD, SUB, MUL, NEG, STORE, EMIT = range(7)
CELL, CONST, TMP = range(3)
MAX_OPS, MAX_TMPS, MAX_CONSTS = 4096, 8, 256


def read_cell(dom, cols, col, row, i):
    """column `col` at trace-row offset `row` seen from LDE row i; a short (periodic) column wraps at its own length,
    which divides N"""
    c = cols[col]
    return c[R2.frame_row(dom, i, row) % len(c)]


def run(ops, dom, cols, consts, i):
    """the op list at LDE row i -> {constraint: value}.  ops: iterable of (op, src, index, row)."""
    p = dom.p
    acc, tmp, out = None, [None] * MAX_TMPS, {}
    for op, src, index, row in ops:
        op, src, index, row = int(op), int(src), int(index), int(row)
        if op <= MUL:
            s = read_cell(dom, cols, index, row, i) if src == CELL else consts[index] if src == CONST else tmp[index]
            assert s is not None and (op == LOAD or acc is not None)
            acc = s if op == LOAD else (acc + s) % p if op == ADD else (acc - s) % p if op == SUB else acc * s % p
        elif op == NEG:
            acc = -acc % p
        elif op == STORE:
            tmp[index] = acc
        else:
            assert op == EMIT and index not in out
            out[index] = acc
    return out


def run_all(ops, dom, cols, consts, n_transitions):
    """-> [T_0, T_1, ...], N values each"""
    ops = [tuple(int(x) for x in o) for o in ops]
    rows = [run(ops, dom, cols, consts, i) for i in range(dom.N)]
    return [[r[c] for r in rows] for c in range(n_transitions)]


def evaluate(expr, dom, cols, consts, i):
    """the expression tree of lambda_elliptic_curves_amd.stark (Expr) at LDE row i, directly"""
    p = dom.p
    memo = {}

    def ev(e):
        if id(e) in memo:
            return memo[id(e)]
        if e.kind == "cell":
            v = read_cell(dom, cols, e.a, e.b, i)
        elif e.kind == "const":
            v = consts[e.a]
        elif e.kind == "neg":
            v = -ev(e.a) % p
        else:
            x, y = ev(e.a), ev(e.b)
            v = (x + y) % p if e.kind == "add" else (x - y) % p if e.kind == "sub" else x * y % p
        memo[id(e)] = v
        return v

    return ev(expr)


def edge_values(p):
    """0, 1, p - 1 and the all-ones 256-bit word reduced mod p"""
    return [0, 1, p - 1, ((1 << 256) - 1) % p]


def fill(p, n, seed, edge=False):
    """n canonical values: random, or drawn from edge_values"""
    rng = np.random.default_rng(seed)
    if edge:
        ev = edge_values(p)
        return [ev[int(k)] for k in rng.integers(0, 4, n)]
    return [int.from_bytes(rng.bytes(32), "big") % p for _ in range(n)]


# ---- the reference's example AIRs as expressions: name -> (builder(stark) -> [expr], columns, constants,
#      {column: period} of the periodic ones)

def _fib2(S):            # fibonacci_2_cols_shifted.rs
    return [S.cell(0, 1) - S.cell(1), S.cell(1, 1) - S.cell(0) - S.cell(1)]


def _simple_fib(S):      # simple_fibonacci.rs
    return [S.cell(0, 2) - S.cell(0, 1) - S.cell(0)]


def _quadratic(S):       # quadratic_air.rs
    return [S.cell(0, 1) - S.cell(0) * S.cell(0)]


def _rom(S):             # read_only_memory.rs; columns a, v, a_sorted, v_sorted, p; constants 1, z, alpha
    one, z, alpha = S.const(0), S.const(1), S.const(2)
    step = S.cell(2, 1) - S.cell(2) - one          # a_sorted' - a_sorted - 1: the same object in both constraints
    return [(S.cell(2, 1) - S.cell(2)) * step,
            (S.cell(3, 1) - S.cell(3)) * step,
            (z - (S.cell(2, 1) + alpha * S.cell(3, 1))) * S.cell(4, 1) - (z - (S.cell(0, 1) + alpha * S.cell(1, 1))) * S.cell(4)]


def _fib_rap(S):         # fibonacci_rap.rs; columns a, b, z; constant gamma
    gamma = S.const(0)
    return [S.cell(2, 1) * (S.cell(1) + gamma) - S.cell(2) * (S.cell(0) + gamma)]


def _periodic(S):        # simple_periodic_cols.rs; columns a, s (s periodic)
    return [S.cell(1) * (S.cell(0, 2) - S.cell(0, 1) - S.cell(0))]


AIRS = {
    "fib2": (_fib2, 2, 0, {}),
    "simple_fib": (_simple_fib, 1, 0, {}),
    "quadratic": (_quadratic, 1, 0, {}),
    "rom": (_rom, 5, 3, {}),
    "fib_rap": (_fib_rap, 3, 1, {}),
    "periodic": (_periodic, 2, 0, {1: 2}),
}


def air_case(name, p, log2_trace, log2_blowup, seed, edge=False):
    """-> (dom, canonical columns (a periodic one has period * blowup elements), col_log2_len or None, constants)"""
    _build, n_cols, n_consts, periodic = AIRS[name]
    dom = R2.Domain(p, log2_trace, log2_blowup, 3)
    lens = [periodic[c] * dom.blowup if c in periodic else dom.N for c in range(n_cols)]
    cols = [fill(p, ln, seed + c, edge) for c, ln in enumerate(lens)]
    consts = fill(p, n_consts, seed + 50, edge)
    if name == "rom":
        consts[0] = 1
    return dom, cols, ([ln.bit_length() - 1 for ln in lens] if periodic else None), consts


def all_temporaries(S, depth=MAX_TMPS):
    """an expression that has `depth` temporaries alive at once: (((c * r_{d-1}) * ...) * r_1) * r_0 with every right
    operand r_k compound.  r_0 is computed first and kept while the left operand is computed, which keeps r_1, ..."""
    e = S.cell(0, depth)
    for k in reversed(range(depth)):
        e = e * (S.cell(0, k) + S.cell(1, k))
    return e
