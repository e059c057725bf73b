"""AIR transition programs without a GPU: the expression compiler of stark.py against the direct evaluation of the
expression trees (both in Python integers, tests/air_program_ref.py), the host-side validation of the C entry points one
bad field at a time, and the validator header alone under AddressSanitizer + UBSan."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from oracle import bigint_def as D
from tests import air_program_ref as A
from tests import stark_round2_ref as R2

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODULI = {"stark252": D.P_STARK252, "fr381": D.P_FR381}


def S():
    from lambda_elliptic_curves_amd import stark
    return stark


def ops_of(program):
    return [tuple(int(x) for x in o) for o in program.ops]


# ---- the compiler

@pytest.mark.parametrize("edge", [False, True], ids=["random", "edge"])
@pytest.mark.parametrize("name", sorted(A.AIRS))
@pytest.mark.parametrize("field", ["stark252", "fr381"])
def test_compiled_ops_agree_with_the_expression_trees(field, name, edge):
    p = MODULI[field]
    exprs = A.AIRS[name][0](S())
    program = S().compile_transitions(exprs)
    dom, cols, _lens, consts = A.air_case(name, p, 3, 2, 7, edge)
    assert program.n_transitions == len(exprs) and program.n_cols == A.AIRS[name][1] and program.n_consts == A.AIRS[name][2]
    ops = ops_of(program)
    for i in range(dom.N):
        got = A.run(ops, dom, cols, consts, i)
        assert got == {c: A.evaluate(e, dom, cols, consts, i) for c, e in enumerate(exprs)}, (name, i)


def test_compiler_output_for_the_stone_case_is_the_obvious_program():
    program = S().compile_transitions(A.AIRS["fib2"][0](S()))
    assert ops_of(program) == [(A.LOAD, A.CELL, 0, 1), (A.SUB, A.CELL, 1, 0), (A.EMIT, 0, 0, 0),
                               (A.LOAD, A.CELL, 1, 1), (A.SUB, A.CELL, 0, 0), (A.SUB, A.CELL, 1, 0), (A.EMIT, 0, 1, 0)]
    assert program.n_tmps == 0 and program.n_mul == 0 and len(program) == 7


def test_a_shared_subexpression_is_computed_once():
    """read-only memory: a_sorted' - a_sorted - 1 is one object in two constraints"""
    program = S().compile_transitions(A.AIRS["rom"][0](S()))
    ops = ops_of(program)
    sub_one = [k for k, o in enumerate(ops) if o[:3] == (A.SUB, A.CONST, 0)]
    assert len(sub_one) == 1
    assert ops[sub_one[0] + 1][0] == A.STORE
    slot = ops[sub_one[0] + 1][2]
    assert sum(1 for o in ops if o[:3] == (A.MUL, A.TMP, slot)) == 2
    # x * x with x compound: stored once, loaded and multiplied from the same slot
    st = S()
    x = st.cell(0) + st.cell(1)
    assert ops_of(st.compile_transitions([x * x])) == [(A.LOAD, A.CELL, 0, 0), (A.ADD, A.CELL, 1, 0), (A.STORE, 0, 0, 0),
                                                      (A.LOAD, A.TMP, 0, 0), (A.MUL, A.TMP, 0, 0), (A.EMIT, 0, 0, 0)]
    # the same expression object as two constraints
    assert ops_of(st.compile_transitions([x, x])) == [(A.LOAD, A.CELL, 0, 0), (A.ADD, A.CELL, 1, 0), (A.STORE, 0, 0, 0), (A.EMIT, 0, 0, 0),
                                                     (A.LOAD, A.TMP, 0, 0), (A.EMIT, 0, 1, 0)]


@pytest.mark.parametrize("edge", [False, True], ids=["random", "edge"])
def test_an_expression_may_use_all_eight_temporaries_and_no_more(edge):
    from lambda_elliptic_curves_amd import errors
    p = MODULI["stark252"]
    e = A.all_temporaries(S(), A.MAX_TMPS)
    program = S().compile_transitions([e])
    assert program.n_tmps == A.MAX_TMPS
    ops = ops_of(program)
    live, most = set(), 0                      # all eight hold a value that is still to be read at one point
    last_read = {}
    for k, o in enumerate(ops):
        if o[0] <= A.MUL and o[1] == A.TMP:
            last_read[o[2]] = k
    for k, o in enumerate(ops):
        if o[0] == A.STORE:
            live.add(o[2])
        most = max(most, len(live))
        live -= {t for t in live if last_read[t] == k}
    assert most == A.MAX_TMPS
    dom = R2.Domain(p, 4, 1, 3)
    cols = [A.fill(p, dom.N, 3, edge), A.fill(p, dom.N, 4, edge)]
    for i in range(dom.N):
        assert A.run(ops, dom, cols, [], i) == {0: A.evaluate(e, dom, cols, [], i)}
    with pytest.raises(errors.InputError):
        S().compile_transitions([A.all_temporaries(S(), A.MAX_TMPS + 1)])


def test_a_program_longer_than_the_limit_is_refused_by_the_compiler():
    from lambda_elliptic_curves_amd import errors
    st = S()

    def line(n):
        e = st.cell(0)
        for k in range(n):
            e = e * st.cell(0, k % 4)
        return e
    assert len(st.compile_transitions([line(A.MAX_OPS - 2)])) == A.MAX_OPS        # LOAD + 4094 MUL + EMIT
    with pytest.raises(errors.InputError):
        st.compile_transitions([line(A.MAX_OPS - 1)])
    with pytest.raises(errors.InputError):
        st.const(A.MAX_CONSTS)
    with pytest.raises(errors.InputError):
        st.compile_transitions([st.cell(0), 5])
    assert len(st.compile_transitions([])) == 0


# ---- the validation of the C entry points: all of it on the host, before any device work

@pytest.fixture(scope="module")
def lib():
    from lambda_elliptic_curves_amd import _lib
    return _lib, _lib.lib()


GOOD = [(A.LOAD, A.CELL, 0, 1), (A.SUB, A.CELL, 1, 0), (A.STORE, 0, 2, 0), (A.MUL, A.CONST, 2, 0), (A.ADD, A.TMP, 2, 0), (A.NEG, 0, 0, 0),
        (A.EMIT, 0, 0, 0)]


def with_op(k, o):
    ops = list(GOOD)
    ops[k] = o
    return ops


# (what, ops, n_transitions, the words lw_hip_last_error must contain)
BAD_PROGRAMS = [
    ("unknown op", with_op(5, (7, 0, 0, 0)), 1, "op 5: unknown op 7"),
    ("unknown src", with_op(1, (A.SUB, 3, 1, 0)), 1, "op 1: unknown src 3"),
    ("column out of range", with_op(1, (A.SUB, A.CELL, 2, 0)), 1, "op 1: column 2 of 2"),
    ("constant out of range", with_op(3, (A.MUL, A.CONST, 3, 0)), 1, "op 3: constant 3 of 3"),
    ("temporary out of range, read", with_op(4, (A.ADD, A.TMP, 8, 0)), 1, "op 4: temporary 8 of 8"),
    ("temporary out of range, stored", with_op(2, (A.STORE, 0, 8, 0)), 1, "op 2: temporary 8 of 8"),
    ("row = n", with_op(0, (A.LOAD, A.CELL, 0, 8)), 1, "op 0: row offset 8"),
    ("NEG with src", with_op(5, (A.NEG, 1, 0, 0)), 1, "op 5: NEG"),
    ("NEG with index", with_op(5, (A.NEG, 0, 1, 0)), 1, "op 5: NEG"),
    ("NEG with row", with_op(5, (A.NEG, 0, 0, 1)), 1, "op 5: NEG"),
    ("first reader of acc is ADD", with_op(0, (A.ADD, A.CELL, 0, 1)), 1, "op 0: the accumulator is read before the first LOAD"),
    ("first reader of acc is EMIT", [(A.EMIT, 0, 0, 0)], 1, "op 0: the accumulator is read before the first LOAD"),
    ("TMP before its STORE", with_op(4, (A.ADD, A.TMP, 1, 0)), 1, "op 4: temporary 1 is read before it is stored"),
    ("EMIT index = n_transitions", with_op(6, (A.EMIT, 0, 1, 0)), 1, "op 6: constraint 1 of 1"),
    ("emitted twice", GOOD + [(A.EMIT, 0, 0, 0)], 1, "op 7: constraint 0 is emitted twice"),
    ("never emitted", GOOD, 2, "op 7 (the end of the program): constraint 1 of 2 is never emitted"),
    ("no ops, one constraint", [], 1, "constraint 0 of 1 is never emitted"),
    ("one op too many", [(A.LOAD, A.CELL, 0, 0)] + [(A.ADD, A.CELL, 0, 0)] * (A.MAX_OPS - 1) + [(A.EMIT, 0, 0, 0)], 1, "4097 ops"),
]


class Call:
    """lw_stark_transition_evaluations_device / lw_stark_transition_evaluations on host memory: trace 2^3, blow-up 4, two
    columns, three constants; every argument can be replaced"""

    def __init__(self, L, dll):
        self.L, self.dll = L, dll
        self.buf = np.zeros((3 * 32 + 3, 4), np.uint64)
        base = (self.buf.ctypes.data + 15) & ~15
        self.cols = (C.c_void_p * 2)(base, base + 32 * 32)
        self.out = base + 64 * 32
        self.consts = np.zeros((257, 4), np.uint64)

    def ops(self, ops):
        arr = (self.L.StarkAirOp * max(1, len(ops)))()
        for k, (op, src, index, row) in enumerate(ops):
            arr[k].op, arr[k].src, arr[k].index, arr[k].row = op, src, index, row
        return arr

    def device(self, ops=GOOD, n_transitions=1, field=None, n_consts=3, consts="own", cols="own", lens=None, n_cols=2, log2_trace=3,
               log2_blowup=2, out="own", stride=0, null_ops=False):
        field = self.L.FIELD_STARK252 if field is None else field
        return self.dll.lw_stark_transition_evaluations_device(
            field, None if null_ops else self.ops(ops), len(ops), self.consts.ctypes.data_as(C.c_void_p) if consts == "own" else consts,
            n_consts, self.cols if cols == "own" else cols, lens, n_cols, log2_trace, log2_blowup, n_transitions,
            C.c_void_p(self.out) if out == "own" else out, stride, None)

    def host(self, ops=GOOD, n_transitions=1, field=None, n_consts=3, columns="own", out="own", log2_trace=3, log2_blowup=2):
        field = self.L.FIELD_STARK252 if field is None else field
        return self.dll.lw_stark_transition_evaluations(
            field, self.ops(ops), len(ops), self.consts.ctypes.data_as(C.c_void_p), n_consts,
            C.c_void_p(self.buf.ctypes.data) if columns == "own" else columns, None, 2, log2_trace, log2_blowup, n_transitions,
            C.c_void_p(self.out) if out == "own" else out)


@pytest.fixture(scope="module")
def call(lib):
    return Call(*lib)


def test_new_entry_points_are_exported(lib):
    L, dll = lib
    for name in ("lw_stark_transition_evaluations_device", "lw_stark_transition_evaluations"):
        assert name in L.EXPORTS
        getattr(dll, name)
    assert C.sizeof(L.StarkAirOp) == 8 and S().AIR_OP_DTYPE.itemsize == 8
    assert (L.AIR_MAX_OPS, L.AIR_MAX_TMPS, L.AIR_MAX_CONSTS) == (A.MAX_OPS, A.MAX_TMPS, A.MAX_CONSTS)
    header = open(os.path.join(ROOT, "include", "lw_hip.h")).read()
    for name, val in (("OPS", A.MAX_OPS), ("TMPS", A.MAX_TMPS), ("CONSTS", A.MAX_CONSTS)):
        assert "#define LW_STARK_AIR_MAX_%s %d\n" % (name, val) in header


@pytest.mark.parametrize("what,ops,n_transitions,words", BAD_PROGRAMS, ids=[b[0] for b in BAD_PROGRAMS])
def test_a_malformed_program_is_a_bad_argument_that_names_the_op(lib, call, what, ops, n_transitions, words):
    L, _dll = lib
    assert call.device(ops, n_transitions) == L.ERR_BAD_ARG
    assert words in L.last_error(), L.last_error()
    assert call.host(ops, n_transitions) == L.ERR_BAD_ARG
    assert words in L.last_error(), L.last_error()


def test_argument_checks_of_the_transition_evaluations(lib, call):
    L, _dll = lib
    bad = L.ERR_BAD_ARG
    assert call.device([], 0) == L.OK and call.host([], 0) == L.OK                  # nothing to write: no device needed
    assert call.device([], 0, cols=None, n_cols=0, consts=None, n_consts=0, out=None) == L.OK
    assert call.device(field=L.FIELD_BABYBEAR) == bad and call.host(field=L.FIELD_BABYBEAR) == bad
    assert call.device(n_consts=257) == bad and "257 constants" in L.last_error()
    assert call.device(consts=None) == bad and call.device(null_ops=True) == bad
    assert call.device(cols=None) == bad and call.device(out=None) == bad
    assert call.host(columns=None) == bad and call.host(out=None) == bad
    assert call.device(out=C.c_void_p(call.out + 8)) == bad                          # misaligned output
    assert call.device(cols=(C.c_void_p * 2)(call.cols[0], call.cols[1] + 8)) == bad and "column 1" in L.last_error()
    assert call.device(cols=(C.c_void_p * 2)(call.cols[0], None)) == bad and "column 1" in L.last_error()
    assert call.device(log2_trace=30, log2_blowup=30) == bad and call.host(log2_trace=30, log2_blowup=30) == bad
    assert call.device(field=L.FIELD_BLS12_381_FR, log2_trace=20, log2_blowup=13) == bad   # beyond the two-adicity
    assert call.device(lens=(C.c_uint32 * 2)(5, 6)) == bad and "column 1" in L.last_error()   # longer than the LDE
    two = GOOD + [(A.EMIT, 0, 1, 0)]
    assert call.device(two, 2, stride=31) == bad and "stride" in L.last_error()


def test_python_layer_checks_lengths_before_the_call():
    from lambda_elliptic_curves_amd import errors, fft
    st = S()
    program = st.compile_transitions(A.AIRS["rom"][0](st))
    cols = [np.zeros((32, 4), np.uint64)] * 5
    with pytest.raises(errors.LengthMismatch):      # two constants for a program that reads three
        st.transition_evaluations(fft.Stark252PrimeField, program, np.zeros((2, 4), np.uint64), cols, 3, 2)
    with pytest.raises(errors.LengthMismatch):      # four columns for five
        st.transition_evaluations(fft.Stark252PrimeField, program, np.zeros((3, 4), np.uint64), cols[:4], 3, 2)
    with pytest.raises(errors.LengthMismatch):      # a column of the wrong length
        st.transition_evaluations(fft.Stark252PrimeField, program, np.zeros((3, 4), np.uint64), cols[:4] + [np.zeros((16, 4), np.uint64)], 3, 2)
    empty = st.compile_transitions([])
    assert st.transition_evaluations(fft.Stark252PrimeField, empty, None, [], 3, 2).shape == (0, 32, 4)


# ---- the validator header alone, under sanitizers

def test_validator_header_under_asan_ubsan(tmp_path):
    exe = tmp_path / "air_program_host"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wno-format-security", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-o", str(exe), os.path.join(ROOT, "tests", "air_program_host_main.cpp")])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.strip() == "ok", (out.returncode, out.stdout[-2000:], out.stderr[-2000:])
