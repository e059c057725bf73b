"""Seeded generators of AIR transition programs for the tests of the five device interpreters (csrc/stark_air.hip, the fused
passes of csrc/ext_round2.cuh and their RAP form, csrc/circle_round2.cuh) and of stark.compile_transitions:

  random_exprs  stark.Expr DAGs that share sub-expressions across constraints, for the compiler;
  random_ops    raw op lists, valid by construction, that reach what the compiler never emits.

Both draw from a numpy Generator (np.random.default_rng(seed)) and nothing else, so a seed names a program.  No GPU.
The seed lists and the shapes of the CPU and the GPU tests are here too, so that both run the same programs."""
import functools
import os

import numpy as np

from tests import air_program_ref as A
from tests import ext_rap_ref as R

XCELL, XCONST = R.XCELL, R.XCONST
BINARY = {"add": A.ADD, "sub": A.SUB, "mul": A.MUL}

# what the tests run: 12 programs per backend at trace 2^3, blow-up 4 (N = 32: under one block, every row offset wraps) and 2
# at trace 2^8, blow-up 4 (N = 1024: four blocks, the wrap crosses a block), the latter capped at about 200 ops
SMALL, LARGE = (3, 2), (8, 2)
SMALL_SEEDS, LARGE_SEEDS = list(range(100, 112)), [200, 201]
LARGE_MAX_OPS = 200
N_COLS, N_CONSTS, N_XCOLS, N_XCONSTS = 3, 4, 2, 2


def extra_seeds():
    """LW_AIR_RANDOM_EXTRA_SEEDS=K: K further seeds at the small shape, for a longer campaign"""
    k = int(os.environ.get("LW_AIR_RANDOM_EXTRA_SEEDS", "0") or 0)
    return list(range(1000, 1000 + k))


def row_offsets(n):
    return sorted({0, 1, 2, n // 2, n - 1})


# ---- expressions for the compiler

class _Exprs:
    """Grows expressions under a budget of temporaries.  The compiler needs, for a tree e (stark.compile_transitions):
    need(leaf) = 0, need(-a) = need(a), need(a op b) = need(a) when b is a leaf, max(need(b), 1 + need(a)) when b is
    compound (b is computed first and kept while a is); a compound object used twice takes one more for as long as it
    lives.  The budget is the 8 of the interpreters less the shared objects of the pool, so most draws compile; the
    estimate is not exact where a pool member is first met deep inside another, and such a draw is refused."""

    def __init__(self, rng, S, n_cols, n_consts, n, n_xcols, n_xconsts, max_shared):
        self.rng, self.S, self.n = rng, S, n
        self.n_cols, self.n_consts, self.n_xcols, self.n_xconsts = n_cols, n_consts, n_xcols, n_xconsts
        self.rows = row_offsets(n)
        self.max_shared = max_shared
        self.pool = []            # compound objects that may be used again: each holds a temporary while it lives
        self.need = {}            # id -> temporaries its first computation takes
        self.nodes = []           # every compound node made, so that the objects outlive the ids

    def pick(self, seq):
        return seq[int(self.rng.integers(0, len(seq)))]

    def chance(self, p):
        return float(self.rng.random()) < p

    def leaf(self):
        kinds = ["cell"] * 3 + (["const"] if self.n_consts else []) + (["xcell"] * 2 if self.n_xcols else []) + (["xconst"] if self.n_xconsts else [])
        kind = self.pick(kinds)
        if kind == "cell":
            return self.S.cell(int(self.rng.integers(0, self.n_cols)), self.pick(self.rows))
        if kind == "const":
            return self.S.const(int(self.rng.integers(0, self.n_consts)))
        if kind == "xcell":
            return self.S.xcell(int(self.rng.integers(0, self.n_xcols)), self.pick(self.rows))
        return self.S.xconst(int(self.rng.integers(0, self.n_xconsts)))

    def made(self, e, need):
        self.need[id(e)] = need
        self.nodes.append(e)
        return e

    def need_of(self, e):
        return 0 if e.is_leaf else self.need[id(e)]

    def binary(self, a, b, kind=None):
        e = a._bin(kind or self.pick(sorted(BINARY)), b)
        if b.is_leaf:
            return self.made(e, self.need_of(a))
        own = 0 if any(b is s for s in self.pool) else 1       # a member of the pool is kept in the slot it has anyway
        return self.made(e, max(self.need_of(b), own + self.need_of(a)))

    def shared(self, budget):
        fits = [e for e in self.pool if self.need_of(e) <= budget]
        return self.pick(fits) if fits else None

    def operand(self, budget):
        """a leaf, or a member of the pool: the same object again"""
        if self.chance(0.3):
            e = self.shared(budget)
            if e is not None:
                return e
        return self.leaf()

    def gen(self, budget, depth):
        if depth <= 0 or self.chance(0.1):
            return self.operand(budget)
        roll = float(self.rng.random())
        if roll < 0.08:                                        # -a, and -(-a)
            a = self.gen(budget, depth - 1)
            e = self.made(-a, self.need_of(a))
            return self.made(-e, self.need_of(a)) if self.chance(0.5) else e
        if roll < 0.16 and budget >= 1:                        # x - x and x * x on one object
            x = self.gen(budget, depth - 1)
            e = x._bin(self.pick(["sub", "mul"]), x)
            return self.made(e, max(self.need_of(x), 0 if x.is_leaf else 1))
        if budget >= 1 and roll < 0.55:                        # a compound right operand: kept while the left one is computed
            b = self.gen(budget, depth - 1)
            return self.binary(self.gen(budget - (0 if b.is_leaf else 1), depth - 1), b)
        return self.binary(self.gen(budget, depth - 1), self.operand(budget))

    def deep(self, budget):
        """exactly `budget` temporaries alive at once: (((l * r_{d-1}) * ...) * r_0 with every r_k compound"""
        e = self.leaf()
        for _ in range(budget):
            r = self.binary(self.leaf(), self.leaf())
            e = self.binary(e, r if self.chance(0.7) else self.binary(r, self.leaf()))
        return e

    def share(self, e):
        if not e.is_leaf and len(self.pool) < self.max_shared and all(e is not s for s in self.pool):
            self.pool.append(e)


def random_exprs(rng, S, n_cols=N_COLS, n_consts=N_CONSTS, n=8, n_xcols=0, n_xconsts=0, n_exprs=None, depth=None, max_shared=3):
    """-> [stark.Expr]: the constraints of one AIR over cell / const, and xcell / xconst where n_xcols / n_xconsts ask.
    The same Python object is met again in later constraints (a shared sub-expression that lives across an EMIT), x - x and
    x * x are built on one object, -(-x) occurs, right operands nest until every temporary is alive, and one constraint
    is listed twice.  Row offsets are from {0, 1, 2, n / 2, n - 1}."""
    g = _Exprs(rng, S, n_cols, n_consts, n, n_xcols, n_xconsts, int(rng.integers(1, max_shared + 1)))
    n_exprs = int(n_exprs or rng.integers(2, 7))
    depth = int(depth or rng.integers(2, 6))
    out = []
    # the first constraint leaves objects in the pool; they are met again below, so they live across its EMIT
    first = g.gen(8 - g.max_shared, depth)
    out.append(first)
    g.share(first)
    for sub in reversed(g.nodes):
        if g.chance(0.3):
            g.share(sub)
    for c in range(1, n_exprs):
        budget = 8 - len(g.pool)
        roll = float(rng.random())
        if roll < 0.35:
            e = g.deep(budget)                                 # every temporary in use, the pool's included
            if g.pool and g.chance(0.7):
                e = g.binary(e, g.pick(g.pool))
        else:
            e = g.gen(budget, depth)
        out.append(e)
    if g.pool and g.chance(0.8):                               # the pool's objects once more, after everything else
        e = g.leaf()
        for s in g.pool:
            e = g.binary(e, s)
        out.append(e)
    out.insert(int(rng.integers(1, len(out) + 1)), out[0])     # the same expression as two constraints
    return out


def evaluate_typed(expr, ar, source):
    """the tree at one row over ext_rap_ref.Arith (ints of F, tuples of E), directly; source(src, index, row) gives a leaf"""
    memo = {}
    SRC = {"cell": A.CELL, "const": A.CONST, "xcell": XCELL, "xconst": XCONST}

    def ev(e):
        if id(e) not in memo:
            if e.is_leaf:
                v = source(SRC[e.kind], e.a, e.b or 0)
            elif e.kind == "neg":
                v = ar.neg(ev(e.a))
            else:
                v = getattr(ar, e.kind)(ev(e.a), ev(e.b))
            memo[id(e)] = v
        return memo[id(e)]

    return ev(expr)


# ---- raw op lists

def random_ops(rng, n_ops, n_transitions, n_cols=N_COLS, n_consts=N_CONSTS, n=8, n_xcols=0, n_xconsts=0):
    """-> [(op, src, index, row)] of exactly n_ops ops that emits constraints 0 .. n_transitions - 1 once each, in a shuffled
    order, valid by construction (n_ops >= max(2 n_transitions, 1): a LOAD or another op stands in front of every EMIT): the accumulator is live
    before it is read and every temporary is stored before it is read.  Temporary `dead` is stored and never read, `hot`
    is read most often; every STORE picks among all eight, so a temporary is overwritten while it holds the other type;
    LOAD TMP, NEG NEG, EMIT straight after a LOAD and ops after the last EMIT are drawn on purpose."""
    T = int(n_transitions)
    assert n_ops >= max(2 * T, 1)
    chance = lambda p: float(rng.random()) < p
    pick = lambda seq: seq[int(rng.integers(0, len(seq)))]
    rows = row_offsets(n)
    tail = int(rng.integers(1, 4)) if n_ops - 2 * T >= 3 else n_ops - 2 * T
    # EMIT places: never op 0, never adjacent to one another (an op of the body lies between two), `tail` ops after the last
    if T:
        free = n_ops - tail - 2 * T          # body ops beyond the one in front of each EMIT
        cuts = sorted(int(x) for x in rng.integers(0, free + 1, T))
        emit_at = {cuts[k] + 2 * k + 1 for k in range(T)}
        assert len(emit_at) == T and min(emit_at) >= 1 and max(emit_at) <= n_ops - tail - 1
    else:
        emit_at = set()
    order = [int(x) for x in rng.permutation(T)]
    dead, hot = (int(x) for x in rng.permutation(A.MAX_TMPS)[:2])
    stored, ops = [], []
    acc_live, neg_again = False, False
    sources = [A.CELL] * 3 + ([A.CONST] * 2 if n_consts else []) + ([XCELL] * 2 if n_xcols else []) + ([XCONST] if n_xconsts else [])

    def operand():
        readable = [t for t in stored if t != dead]
        if readable and chance(0.35):
            return (A.TMP, hot if hot in readable and chance(0.5) else pick(readable), 0)
        src = pick(sources)
        if src == A.CELL:
            return (src, int(rng.integers(0, n_cols)), pick(rows))
        if src == XCELL:
            return (src, int(rng.integers(0, n_xcols)), pick(rows))
        return (src, int(rng.integers(0, n_consts if src == A.CONST else n_xconsts)), 0)

    for k in range(n_ops):
        if k in emit_at:
            ops.append((A.EMIT, 0, order.pop(), 0))
            continue
        if not acc_live or (k + 1 in emit_at and chance(0.3)):      # the first op; EMIT straight after a LOAD
            ops.append((A.LOAD,) + operand())
            acc_live, neg_again = True, False
            continue
        roll = float(rng.random())
        if neg_again or roll < 0.08:
            ops.append((A.NEG, 0, 0, 0))
            neg_again = not neg_again and chance(0.5)               # NEG NEG
        elif roll < 0.25:
            t = pick([hot, dead] + list(range(A.MAX_TMPS)))
            ops.append((A.STORE, 0, t, 0))
            if t not in stored:
                stored.append(t)
        elif roll < 0.40:
            ops.append((A.LOAD,) + operand())
        else:
            ops.append((pick([A.ADD, A.SUB, A.MUL]),) + operand())
    assert len(ops) == n_ops and not order
    return ops


def raw_shape(rng, max_ops=1100):
    """(n_ops, n_transitions) of one raw program: a length anywhere from the shortest to above 1000 ops, one constraint, a
    few, or at least 65 (two words of the validator's bitmap)"""
    T = [1, 1, int(rng.integers(2, 9)), int(rng.integers(65, 80))][int(rng.integers(0, 4))]
    T = min(T, (max_ops - 1) // 2)
    lo = 2 * T + 1
    hi = [lo + 3, 60, 300, max_ops][int(rng.integers(0, 4))]
    return int(rng.integers(lo, max(lo, min(hi, max_ops)) + 1)), T


# ---- the programs of the tests: seed -> (kind, ops, n_transitions, the expressions or None)

def programs(S, seeds, shape, typed, max_ops=None):
    """One program per seed, the even seeds through the compiler, the odd ones raw; a draw the compiler refuses
    (errors.InputError: more than 8 temporaries or 4096 ops) gives (seed, "refused", None, 0, None).  typed: with the
    sources of E.  Without max_ops the first raw program of a list has more than 1000 ops, the second at least 65
    constraints and the third is the shortest there is with a constraint (LOAD, EMIT), so that every such list reaches
    all three."""
    from lambda_elliptic_curves_amd.errors import InputError
    n = 1 << shape[0]
    xc, xk = (N_XCOLS, N_XCONSTS) if typed else (0, 0)
    out, n_raw = [], 0
    for seed in seeds:
        rng = np.random.default_rng(seed)
        if seed % 2 == 0:
            small = dict(n_exprs=3, depth=3) if max_ops else {}
            exprs = random_exprs(rng, S, n=n, n_xcols=xc, n_xconsts=xk, **small)
            try:
                program = S.compile_transitions(exprs)
            except InputError:
                out.append((seed, "refused", None, 0, None))
                continue
            ops = [tuple(int(x) for x in o) for o in program.ops.tolist()]
            if max_ops and len(ops) > max_ops:
                out.append((seed, "refused", None, 0, None))
                continue
            out.append((seed, "compiled", ops, len(exprs), exprs))
        else:
            n_ops, T = raw_shape(rng, max_ops or 1100)
            if not max_ops and n_raw == 0:
                n_ops, T = int(rng.integers(1001, 1101)), 1
            elif not max_ops and n_raw == 1:
                T = int(rng.integers(65, 80))
                n_ops = max(n_ops, 2 * T + 1 + int(rng.integers(0, 40)))
            elif not max_ops and n_raw == 2:
                n_ops, T = 2, 1
            n_raw += 1
            out.append((seed, "raw", random_ops(rng, n_ops, T, n=n, n_xcols=xc, n_xconsts=xk), T, None))
    return out


@functools.lru_cache(maxsize=None)
def program_lists(S):
    """the four lists of the tests, generated once: (typed, "small" | "large") -> programs(...)"""
    small = SMALL_SEEDS + extra_seeds()
    return {(typed, size): programs(S, seeds, shape, typed, max_ops)
            for typed in (False, True) for size, seeds, shape, max_ops in (("small", small, SMALL, None), ("large", LARGE_SEEDS, LARGE, LARGE_MAX_OPS))}


def descriptors_of(n_transitions, seed):
    """two or three distinct zerofier descriptors over the constraints (the fused passes take 8 classes a call)"""
    kinds = [dict(period=1, offset=0, end_exemptions=1), dict(period=2, offset=1, end_exemptions=1), dict(period=1, offset=0, end_exemptions=2)]
    k = 2 + seed % 2
    return [dict(kinds[(c + seed) % k]) for c in range(n_transitions)]
