"""The generators of tests/air_program_gen.py without a GPU, over the very seed lists tests/test_gpu_air_program_random.py
runs: what stark.compile_transitions makes of a random DAG is the DAG (the op list run by the Python interpreters against
the direct evaluation of the trees, in Stark252 and, typed, over Fp2 and Fp4), every program passes the host check of
csrc/air_program.h with the typing of ext_rap_ref.type_program (the stand-alone program of tests/test_ext_rap_cpu.py, under
the sanitizers), the compiler refuses at most a quarter of the draws, and the lists cover what they are there for."""
import numpy as np
import pytest

from oracle import bigint_def as D
from tests import air_program_gen as G
from tests import air_program_ref as A
from tests import ext_rap_ref as R
from tests import ext_round2_ref as M
from tests import stark_round2_ref as R2
from tests.test_ext_rap_cpu import check_program, exe   # noqa: F401  (exe: the module's fixture, built once here too)

FIELDS = ["gl2", "bb4"]
SHAPES = {"small": G.SMALL, "large": G.LARGE}


def S():
    from lambda_elliptic_curves_amd import stark
    return stark


def lists(typed=None):
    """[(typed, size, seed, kind, ops, n_transitions, exprs)] of every program that compiled or was drawn raw"""
    return [(t, size) + entry for (t, size), entries in G.program_lists(S()).items() for entry in entries
            if entry[1] != "refused" and (typed is None or t == typed)]


def rows_of(N):
    return [0, N // 2 + 1, N - 1]


def test_the_compiler_refuses_at_most_a_quarter_of_the_draws():
    drawn = [e for entries in G.program_lists(S()).values() for e in entries if e[0] % 2 == 0]
    refused = [e[0] for e in drawn if e[1] == "refused"]
    assert len(drawn) >= 2 * (len(G.SMALL_SEEDS) + len(G.LARGE_SEEDS)) // 2
    assert 4 * len(refused) <= len(drawn), refused
    for (typed, size), entries in G.program_lists(S()).items():       # and in every list on its own
        mine = [e for e in entries if e[0] % 2 == 0]
        assert 4 * sum(1 for e in mine if e[1] == "refused") <= len(mine), (typed, size)
        assert len(entries) == len(G.LARGE_SEEDS if size == "large" else G.SMALL_SEEDS + G.extra_seeds())
        if size == "large":
            assert all(len(e[2]) <= G.LARGE_MAX_OPS for e in entries if e[2] is not None)


def test_compiled_programs_are_their_expressions():
    p = D.P_STARK252
    n_checked = 0
    for _t, size, seed, kind, ops, T, exprs in lists(typed=False):
        if kind != "compiled":
            continue
        dom = R2.Domain(p, SHAPES[size][0], SHAPES[size][1], 3)
        cols = [A.fill(p, dom.N, seed + c, edge=(seed % 4 == 2)) for c in range(G.N_COLS)]
        consts = A.fill(p, G.N_CONSTS, seed + 50)
        assert T == len(exprs)
        for i in rows_of(dom.N):
            assert A.run(ops, dom, cols, consts, i) == {c: A.evaluate(e, dom, cols, consts, i) for c, e in enumerate(exprs)}, (seed, i)
        n_checked += 1
    assert n_checked >= 6


@pytest.mark.parametrize("field", FIELDS)
def test_typed_compiled_programs_are_their_expressions(field):
    F = M.FIELDS[field]
    ar = R.Arith(F)
    n_checked = 0
    for _t, size, seed, kind, ops, T, exprs in lists(typed=True):
        if kind != "compiled":
            continue
        dom = M.domain(F, SHAPES[size][0], SHAPES[size][1], 3)
        rng = np.random.default_rng(seed)
        word = lambda: int.from_bytes(rng.bytes(16), "big") % F.p
        cols = [[word() for _ in range(dom.N)] for _ in range(G.N_COLS)]
        aux = [[tuple(word() for _ in range(F.width)) for _ in range(dom.N)] for _ in range(G.N_XCOLS)]
        consts = [word() for _ in range(G.N_CONSTS)]
        xconsts = [tuple(word() for _ in range(F.width)) for _ in range(G.N_XCONSTS)]
        for i in rows_of(dom.N):
            def source(src, index, row):
                if src == A.CELL:
                    return A.read_cell(dom, cols, index, row, i)
                if src == R.XCELL:
                    return aux[index][R2.frame_row(dom, i, row) % dom.N]
                return consts[index] if src == A.CONST else xconsts[index]
            got = R.run(F, ops, source, ar)
            assert got == {c: G.evaluate_typed(e, ar, source) for c, e in enumerate(exprs)}, (seed, i)
        n_checked += 1
    assert n_checked >= 6


def one_op_program():
    """the shortest program there is: one LOAD, no constraint"""
    return G.random_ops(np.random.default_rng(1), 1, 0)


@pytest.mark.parametrize("field", FIELDS)
def test_every_program_passes_the_host_check_with_the_models_typing(exe, field):   # noqa: F811
    F = M.FIELDS[field]
    cases = [(t, size, seed, ops, T) for t, size, seed, _kind, ops, T, _e in lists()] + [(False, "small", -1, one_op_program(), 0)]
    assert len(cases) >= 28
    for typed, size, seed, ops, T in cases:
        words, n_tmps, n_ext, slots = R.type_program(ops, F.width)
        got = check_program(exe, field, ops, n_consts=G.N_CONSTS, n_xconsts=G.N_XCONSTS if typed else 0, n_cols=G.N_COLS, n_xcols=G.N_XCOLS if typed else 0,
                            log2_trace=SHAPES[size][0], log2_lde=sum(SHAPES[size]), n_transitions=T)
        assert got[0] == f"ok {n_tmps} {n_ext} {slots}", (typed, size, seed, got)
        assert [int(w) for w in got[1].split()] == words, (typed, size, seed)
        if not typed:
            assert n_ext == 0 and slots == n_tmps and words == [op | src << 8 | index << 16 | row << 32 for op, src, index, row in ops]


# ---- what the lists are there for

def typed_events(ops):
    """[(op, accumulator in E before the op, operand in E)] and the retypings [(temporary, was in E, is in E)]"""
    acc_ext, tmp_ext, events, retyped = False, {}, [], []
    for op, src, index, _row in ops:
        if op <= A.MUL:
            src_ext = src in (R.XCELL, R.XCONST) or (src == A.TMP and tmp_ext[index])
            events.append((op, acc_ext if op != A.LOAD else None, src_ext))
            acc_ext = src_ext if op == A.LOAD else acc_ext or src_ext
        else:
            events.append((op, acc_ext, None))
            if op == A.STORE:
                if index in tmp_ext and tmp_ext[index] != acc_ext:
                    retyped.append((index, tmp_ext[index], acc_ext))
                tmp_ext[index] = acc_ext
    return events, retyped


def most_alive(ops):
    """the most temporaries that hold a value still to be read, at one point"""
    live, most = set(), 0
    reads_left = {}
    for k, o in enumerate(ops):
        if o[0] <= A.MUL and o[1] == A.TMP:
            reads_left.setdefault(o[2], []).append(k)
    last = {}
    for k, o in enumerate(ops):         # a value's last read: the last read of the slot before the slot's next STORE
        if o[0] == A.STORE:
            last[k] = max([r for r in reads_left.get(o[2], []) if r > k and not any(ops[j][0] == A.STORE and ops[j][2] == o[2] for j in range(k + 1, r))], default=None)
    alive = {}
    for k, o in enumerate(ops):
        if o[0] == A.STORE and last[k] is not None:
            alive[o[2]] = last[k]
        most = max(most, len(alive))
        alive = {t: end for t, end in alive.items() if end > k}
    return most


def test_coverage_of_the_plain_lists():
    progs = lists(typed=False)
    pairs = {(o[0], o[1]) for *_x, ops, _T, _e in progs for o in ops if o[0] <= A.MUL}
    assert pairs == {(op, src) for op in (A.LOAD, A.ADD, A.SUB, A.MUL) for src in (A.CELL, A.CONST, A.TMP)}
    compiled = [(ops, T) for *_x, kind, ops, T, _e in progs if kind == "compiled"]
    raw = [(ops, T) for *_x, kind, ops, T, _e in progs if kind == "raw"]
    assert any(S().AirProgram(np.array(ops, dtype=S().AIR_OP_DTYPE), T).n_tmps == A.MAX_TMPS and most_alive(ops) == A.MAX_TMPS for ops, T in compiled)
    # a kept sub-expression read after an EMIT that followed its STORE, in a program with all eight alive at once
    def kept_across_an_emit(ops):
        for k, o in enumerate(ops):
            if o[0] == A.STORE:
                emit = False
                for q in ops[k + 1:]:
                    if q[0] == A.STORE and q[2] == o[2]:
                        break
                    emit = emit or q[0] == A.EMIT
                    if emit and q[0] <= A.MUL and q[1] == A.TMP and q[2] == o[2]:
                        return True
        return False
    assert any(kept_across_an_emit(ops) and most_alive(ops) == A.MAX_TMPS for ops, _T in compiled)
    # the expressions: x - x and x * x on one object, -(-x), one object as two constraints, every row offset
    exprs = [e for *_x, kind, _ops, _T, es in progs if kind == "compiled" for e in es]
    seen, kinds, rows = set(), set(), set()
    stack = list(exprs)
    while stack:
        e = stack.pop()
        if id(e) in seen:
            continue
        seen.add(id(e))
        if e.kind == "cell":
            rows.add(e.b)
        if e.is_leaf:
            continue
        if e.kind == "neg":
            kinds.add("neg neg" if e.a.kind == "neg" else "neg")
            stack.append(e.a)
        else:
            if e.a is e.b and not e.a.is_leaf:
                kinds.add("same " + e.kind)
            stack += [e.a, e.b]
    assert {"neg neg", "same sub", "same mul"} <= kinds
    assert rows == set(G.row_offsets(8)) | set(G.row_offsets(256))
    assert all(any(es[j] is es[k] for j in range(len(es)) for k in range(j)) for *_x, kind, _ops, _T, es in progs if kind == "compiled")
    # the raw programs: what the compiler never emits
    flat = lambda ops: "".join("LASMNTE"[o[0]] for o in ops)
    assert any("NN" in flat(ops) for ops, _T in raw) and any("LE" in flat(ops) for ops, _T in raw)
    assert any(o[0] == A.LOAD and o[1] == A.TMP for ops, _T in raw for o in ops)
    assert any(ops[-1][0] != A.EMIT for ops, _T in raw)
    assert not any(ops[-1][0] != A.EMIT for ops, _T in compiled)
    for ops, T in raw:
        emitted = [o[2] for o in ops if o[0] == A.EMIT]
        assert sorted(emitted) == list(range(T))
    assert any([o[2] for o in ops if o[0] == A.EMIT] != list(range(T)) and T >= 65 for ops, T in raw)
    assert {T for _ops, T in raw} >= {1} and min(len(ops) for ops, _T in raw) == 2 and max(len(ops) for ops, _T in raw) > 1000
    stored_never_read = lambda ops: {o[2] for o in ops if o[0] == A.STORE} - {o[2] for o in ops if o[0] <= A.MUL and o[1] == A.TMP}
    assert any(stored_never_read(ops) for ops, _T in raw)
    assert any(sum(1 for o in ops if o[0] <= A.MUL and o[1] == A.TMP and o[2] == t) >= 3 for ops, _T in raw for t in range(A.MAX_TMPS))


def test_coverage_of_the_typed_lists():
    progs = lists(typed=True)
    pairs = {(o[0], o[1]) for *_x, ops, _T, _e in progs for o in ops if o[0] <= A.MUL}
    assert pairs == {(op, src) for op in (A.LOAD, A.ADD, A.SUB, A.MUL) for src in (A.CELL, A.CONST, A.TMP, R.XCELL, R.XCONST)}
    events, retyped = set(), set()
    for *_x, ops, _T, _e in progs:
        ev, rt = typed_events(ops)
        events |= set(ev)
        retyped |= {(was, now) for _t, was, now in rt}
    assert {(op, a, s) for op in (A.ADD, A.SUB, A.MUL) for a in (False, True) for s in (False, True)} <= events
    assert {(A.LOAD, None, False), (A.LOAD, None, True)} <= events
    assert {(op, a, None) for op in (A.NEG, A.STORE, A.EMIT) for a in (False, True)} <= events
    assert retyped == {(False, True), (True, False)}
    # a temporary that held an element of E, overwritten with a word and read back as a word; and the other way round
    def read_back(ops, was, now):
        tmp_ext, acc_ext, changed = {}, False, set()
        for op, src, index, _row in ops:
            if op <= A.MUL:
                if src == A.TMP and index in changed and tmp_ext[index] == now:
                    return True
                src_ext = src in (R.XCELL, R.XCONST) or (src == A.TMP and tmp_ext[index])
                acc_ext = src_ext if op == A.LOAD else acc_ext or src_ext
            elif op == A.STORE:
                if tmp_ext.get(index) == was and acc_ext == now:
                    changed.add(index)
                elif acc_ext != now:
                    changed.discard(index)
                tmp_ext[index] = acc_ext
        return False
    assert any(read_back(ops, True, False) for *_x, ops, _T, _e in progs)
    assert any(read_back(ops, False, True) for *_x, ops, _T, _e in progs)
    assert any(S().AirProgram(np.array(ops, dtype=S().AIR_OP_DTYPE), T).n_tmps == A.MAX_TMPS and most_alive(ops) == A.MAX_TMPS
               for *_x, kind, ops, T, _e in progs if kind == "compiled")
