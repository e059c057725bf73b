"""The randomized AIR over Goldilocks with Fp2 and BabyBear with Fp4 without a device: every refusal of air_program_check_rap
with its message, the statuses the new entry points (aux_fractions, rap_constraint_evaluations) return before any device
work, which pins the order of their checks, the typing of a program against the model of tests/ext_rap_ref.py, the programs
stark.compile_transitions gives for the existing examples (unchanged), and the host code (the typing check, the packing of
the coefficient lists, the step groups over boundary values in E) compiled for the host with the address and
undefined-behaviour sanitizers (tests/ext_rap_host_main.cpp), run as a child process and compared with Python."""
import hashlib
import os
import subprocess

import numpy as np
import pytest

from tests import air_program_ref as A
from tests import ext_rap_ref as R
from tests import ext_round2_ref as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ["gl2", "bb4"]
NP = {"gl2": np.uint64, "bb4": np.uint32}
BAD_ARG, INV_ZERO, ALLOC = r"\[-9\]", r"\[-10\]", r"\[-6\]"


class Buffer:
    """host memory where the calls expect device memory: the checks under test never follow a pointer"""

    def __init__(self, name, n_words, skew=0):
        self.a = np.zeros(n_words + 4, NP[name])
        self.skew = skew
        self.device = "cpu"

    def data_ptr(self):
        return self.a.ctypes.data + self.skew * self.a.itemsize


def module(name):
    from lambda_elliptic_curves_amd import babybear_ext, goldilocks_ext
    return {"gl2": goldilocks_ext, "bb4": babybear_ext}[name]


def refused(code, text=None):
    from lambda_elliptic_curves_amd import errors
    kind = errors.FieldError if code == INV_ZERO else errors.HipError
    return pytest.raises(kind, match=code + (".*" + text if text else ""))


def program_of(ops, n_transitions):
    from lambda_elliptic_curves_amd import stark
    return stark.AirProgram(np.array(ops, dtype=stark.AIR_OP_DTYPE), n_transitions)


def fib_rap_program():
    from lambda_elliptic_curves_amd import stark
    return stark.compile_transitions(R.RAP_AIRS["fib_rap"][0](stark))


# ---- the leaves and what compile_transitions makes of them
EXISTING = {   # sha256 of the op bytes of every example of air_program_ref, as compiled before the two new leaves existed
    "fib2": (7, "9ecb9e43da1b6e57bcc39d9f9a527ec3a4305ef357ff05163bf064156abeae87"),
    "fib_rap": (13, "31e6f703e3daa5ef1b51060832c821cbb921ce557bef3381b09f01e9e7acfcdd"),
    "periodic": (7, "c0f3797685f6dde41011fcf9ff19d8f4ac40b742e905eb89eac5b86c064a4abf"),
    "quadratic": (6, "53e7e2378eed7fb995311ac1b537e3091b3d3bb12825a3ffca7775059834283a"),
    "rom": (33, "6c4e1d809ff5bb61dfaf0d8c994beb8d1f9c1ebca95e6315be0a1fa628be264f"),
    "simple_fib": (4, "297c68deade837531f4c3947009ca6734cbc0b47157d5ca1a2c4fcf03cacc749"),
    "all_temporaries": (34, "2ab5aeba7856ba9e97529e5701f2d3d28b8f1a2e23f801736a1b4e5eda39b320"),
}


def test_existing_examples_compile_to_the_same_bytes():
    from lambda_elliptic_curves_amd import stark
    assert sorted(EXISTING) == sorted(list(A.AIRS) + ["all_temporaries"])
    for name, (n_ops, digest) in EXISTING.items():
        exprs = [A.all_temporaries(stark)] if name == "all_temporaries" else A.AIRS[name][0](stark)
        program = stark.compile_transitions(exprs)
        assert (len(program), hashlib.sha256(program.ops.tobytes()).hexdigest()) == (n_ops, digest), name
        assert program.n_xcols == 0 and program.n_xconsts == 0


def test_the_new_leaves_compile_to_the_new_sources():
    from lambda_elliptic_curves_amd import errors, stark
    program = fib_rap_program()
    ops = program.ops.tolist()
    assert (A.LOAD, R.XCELL, 0, 1) in ops and (A.LOAD, R.XCONST, 0, 0) in ops and (A.ADD, A.CELL, 1, 0) in ops
    assert (program.n_xcols, program.n_xconsts, program.n_cols, program.n_consts) == (1, 1, 2, 0)
    rom = stark.compile_transitions(R.RAP_AIRS["rom"][0](stark))
    assert (rom.n_xcols, rom.n_xconsts, rom.n_cols, rom.n_consts) == (1, 2, 4, 1)
    for bad in (lambda: stark.xcell(1 << 16), lambda: stark.xcell(0, 1 << 32), lambda: stark.xconst(256), lambda: stark.xconst(-1)):
        with pytest.raises(errors.InputError):
            bad()


# ---- the statuses of the entry points, in the order of their checks
def rap_call(name, program=None, consts=(), xconsts=None, n_cols=2, n_aux=1, log2_trace=4, log2_blowup=2, boundary=None, transitions=None, offset=3,
             out=None, cols=None, aux=None, aux_stride=0):
    F = M.FIELDS[name]
    N = 1 << min(log2_trace + log2_blowup, 10)
    one = F.word_elem(M.lift(F, 1))
    if boundary is None:
        boundary = [(0, 0, one, one, True), (0, 0, F.word(1), one)]
    if transitions is None:
        transitions = [dict(period=1, offset=0, end_exemptions=1, coeff=one)]
    cols = cols if cols is not None else [Buffer(name, N) for _ in range(n_cols)]
    aux = aux if aux is not None else [Buffer(name, F.width * N) for _ in range(n_aux)]
    out = out or Buffer(name, F.width * N)
    off = None if offset is None else F.word(offset)
    return module(name).rap_constraint_evaluations_device(program or fib_rap_program(), list(consts), [one] if xconsts is None else xconsts, cols, aux, log2_trace,
                                                          log2_blowup, boundary, transitions, t_out=out, aux_stride=aux_stride, offset=off, stream=0)


@pytest.mark.parametrize("field", FIELDS)
def test_rap_constraint_evaluations_argument_rules(field):
    F = M.FIELDS[field]
    one = F.word_elem(M.lift(F, 1))
    bad = program_of([(A.LOAD, R.XCELL, 0, 0), (A.MUL, R.XCONST, 0, 1), (A.EMIT, 0, 0, 0)], 1)
    with refused(BAD_ARG, "AIR program: op 1: row 1 on an extension constant operand"):
        rap_call(field, program=bad)
    # the domain before the program, the program before everything below
    with refused(BAD_ARG, "beyond the transform"):
        rap_call(field, program=bad, log2_trace=40)
    with refused(BAD_ARG, "AIR program: op 1"):
        rap_call(field, program=bad, offset=1, out=Buffer(field, 256, skew=1), boundary=[(3, 0, one, one, True)])
    # the boundary entries before the transitions, the buffers and the offset
    with refused(BAD_ARG, "boundary constraint 0: auxiliary column 1 of 1"):
        rap_call(field, boundary=[(1, 0, one, one, True)], transitions=[dict(period=0, coeff=one)])
    with refused(BAD_ARG, "boundary constraint 0: column 2 of 2"):
        rap_call(field, boundary=[(2, 0, one, one)])
    with refused(BAD_ARG, "period 0"):
        rap_call(field, transitions=[dict(period=0, coeff=one)], out=Buffer(field, 256, skew=1))
    # out and the main columns before the auxiliary ones, all of them before the offset
    with refused(BAD_ARG, "16-byte aligned"):
        rap_call(field, out=Buffer(field, 256, skew=1), aux=[Buffer(field, 256, skew=1)])
    with refused(BAD_ARG, "column 1: null or misaligned"):
        rap_call(field, cols=[Buffer(field, 64), Buffer(field, 64, skew=1)], aux_stride=3)
    with refused(BAD_ARG, "auxiliary columns: plane stride 3 below"):
        rap_call(field, aux_stride=3, aux=[Buffer(field, 256, skew=1)])
    with refused(BAD_ARG, "auxiliary column 0: null or misaligned"):
        rap_call(field, aux=[Buffer(field, 256, skew=1)], offset=1)
    shared = Buffer(field, F.width * 64)
    with refused(BAD_ARG, "out overlaps auxiliary column 0"):
        rap_call(field, out=shared, aux=[shared], offset=1)
    with refused(INV_ZERO, "h\\^N = 1"):
        rap_call(field, offset=1)
    with refused(INV_ZERO, "offset is zero"):
        rap_call(field, offset=0)


def test_rap_babybear_words_must_be_below_p():
    F, p = M.BB4, M.BB4.p
    one = F.word_elem(M.lift(F, 1))
    with refused(BAD_ARG, "extension constants: word 2"):
        rap_call("bb4", xconsts=[(0, 0, p, 0)])
    with refused(BAD_ARG, "boundary value: word 3"):
        rap_call("bb4", boundary=[(0, 0, (1, 2, 3, p), one)])          # on a main column: the high coordinates count
    with refused(BAD_ARG, "boundary coefficient"):
        rap_call("bb4", boundary=[(0, 0, one, (p, 0, 0, 0), True)])
    # the program before the words
    with refused(BAD_ARG, "AIR program"):
        rap_call("bb4", program=program_of([(A.ADD, R.XCONST, 0, 0), (A.EMIT, 0, 0, 0)], 1), xconsts=[(0, 0, p, 0)])


@pytest.mark.parametrize("field", FIELDS)
def test_the_plain_entry_still_refuses_the_new_sources(field):
    F = M.FIELDS[field]
    one = F.word_elem(M.lift(F, 1))
    with refused(BAD_ARG, "AIR program: op 0: unknown src 3"):
        module(field).constraint_evaluations_device(program_of([(A.LOAD, R.XCELL, 0, 0), (A.EMIT, 0, 0, 0)], 1), [], [Buffer(field, 64), Buffer(field, 64)], 4, 2, [],
                                                    [dict(coeff=one)], t_out=Buffer(field, F.width * 64), offset=F.word(3), stream=0)
    with refused(BAD_ARG, "AIR program: op 0: unknown src 4"):
        module(field).constraint_evaluations_device(fib_rap_program(), [], [Buffer(field, 64), Buffer(field, 64)], 4, 2, [], [dict(coeff=one)],
                                                    t_out=Buffer(field, F.width * 64), offset=F.word(3), stream=0)


def aux_call(name, n=8, n_cols=2, num=None, den=None, mode=0, cols=None, out=None, out_stride=0, count_zeros=False):
    F = M.FIELDS[name]
    one = F.word_elem(M.lift(F, 1))
    cols = cols if cols is not None else [Buffer(name, 64) for _ in range(n_cols)]
    out = out or Buffer(name, F.width * 64)
    return module(name).aux_fractions_device(cols, n, num or (one, [(0, one)]), den or (one, [(1, one)]), mode=mode, t_out=out, out_stride=out_stride,
                                             count_zeros=count_zeros, stream=0)


@pytest.mark.parametrize("field", FIELDS)
def test_aux_fractions_argument_rules(field):
    F = M.FIELDS[field]
    one = F.word_elem(M.lift(F, 1))
    seventeen = (one, [(0, one)] * 17)
    with refused(BAD_ARG, "no rows"):
        aux_call(field, n=0, mode=9)
    with refused(ALLOC, "rows"):
        aux_call(field, n=(1 << 36) + 1, mode=9)
    with refused(BAD_ARG, "mode 9"):
        aux_call(field, mode=9, num=seventeen)
    with refused(BAD_ARG, "numerator: 17 terms"):
        aux_call(field, num=seventeen, den=seventeen)
    with refused(BAD_ARG, "denominator: 17 terms"):
        aux_call(field, den=seventeen, out=Buffer(field, 256, skew=1))
    with refused(BAD_ARG, "denominator: term 1: column 2 of 2"):
        aux_call(field, den=(one, [(1, one), (2, one)]), out=Buffer(field, 256, skew=1))
    with refused(BAD_ARG, "16-byte aligned"):
        aux_call(field, out=Buffer(field, 256, skew=1), out_stride=3)
    with refused(BAD_ARG, "out: plane stride 3 below the length 8"):
        aux_call(field, out_stride=3, cols=[Buffer(field, 64), Buffer(field, 64, skew=1)])
    with refused(BAD_ARG, "column 1: null or misaligned"):
        aux_call(field, cols=[Buffer(field, 64), Buffer(field, 64, skew=1)])
    shared = Buffer(field, F.width * 64)
    with refused(BAD_ARG, "out overlaps column 0"):
        aux_call(field, cols=[shared, Buffer(field, 64)], out=shared)
    if field == "bb4":
        with refused(BAD_ARG, "numerator: word 1"):
            aux_call(field, num=((0, F.p, 0, 0), []), den=seventeen)
        with refused(BAD_ARG, "denominator: word 6"):
            aux_call(field, den=(one, [(0, one), (1, (0, 0, F.p, 0))]), out=Buffer(field, 256, skew=1))


# ---- the host code under the sanitizers
@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    hipcc = "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        hipcc = "hipcc"
    out = tmp_path_factory.mktemp("ext_rap") / "ext_rap_host"
    subprocess.check_call([hipcc, "-x", "hip", "--cuda-host-only", "-O2", "-std=c++17", "-Xarch_host", "-fsanitize=address,undefined",
                           "-Xarch_host", "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "lambda_elliptic_curves_amd", "csrc"),
                           os.path.join(ROOT, "tests", "ext_rap_host_main.cpp"), "-o", str(out)], timeout=600)
    return str(out)


def host(exe, field, what, words):
    out = subprocess.run([exe, field, what] + [str(int(w)) for w in words], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    return out.stdout.splitlines()


def check_program(exe, field, ops, n_consts=1, n_xconsts=2, n_cols=2, n_xcols=1, log2_trace=4, log2_lde=6, n_transitions=1):
    words = [n_consts, n_xconsts, n_cols, n_xcols, log2_trace, log2_lde, n_transitions, len(ops)]
    for o in ops:
        words += list(o)
    return host(exe, field, "prog", words)


REFUSALS = [
    ([(A.LOAD, R.XCELL, 1, 0), (A.EMIT, 0, 0, 0)], {}, "op 0: auxiliary column 1 of 1"),
    ([(A.LOAD, A.CELL, 0, 0), (A.MUL, R.XCELL, 0, 0), (A.EMIT, 0, 0, 0)], dict(n_xcols=0), "op 1: auxiliary column 0 of 0"),
    ([(A.LOAD, R.XCELL, 0, 16), (A.EMIT, 0, 0, 0)], {}, "op 0: row offset 16 of a trace of 2^4 rows"),
    ([(A.LOAD, R.XCONST, 2, 0), (A.EMIT, 0, 0, 0)], {}, "op 0: extension constant 2 of 2"),
    ([(A.LOAD, A.CELL, 0, 0), (A.SUB, R.XCONST, 0, 1), (A.EMIT, 0, 0, 0)], {}, "op 1: row 1 on an extension constant operand"),
    ([(A.LOAD, 5, 0, 0), (A.EMIT, 0, 0, 0)], {}, "op 0: unknown src 5"),
    ([(A.ADD, R.XCONST, 0, 0), (A.EMIT, 0, 0, 0)], {}, "op 0: the accumulator is read before the first LOAD"),
    ([(A.LOAD, R.XCONST, 0, 0), (A.ADD, A.TMP, 1, 0), (A.EMIT, 0, 0, 0)], {}, "op 1: temporary 1 is read before it is stored"),
    ([(A.LOAD, R.XCONST, 0, 0), (A.STORE, 0, 8, 0), (A.EMIT, 0, 0, 0)], {}, "op 1: temporary 8 of 8"),
    ([(A.LOAD, R.XCONST, 0, 0), (A.EMIT, 0, 0, 0), (A.EMIT, 0, 0, 0)], {}, "op 2: constraint 0 is emitted twice"),
    ([(A.LOAD, R.XCONST, 0, 0)], {}, "op 1 (the end of the program): constraint 0 of 1 is never emitted"),
    ([(A.LOAD, A.CONST, 1, 0), (A.EMIT, 0, 0, 0)], {}, "op 0: constant 1 of 1"),
    ([(A.LOAD, R.XCONST, 0, 0), (A.EMIT, 0, 0, 0)], dict(n_xconsts=257), "257 extension constants: a program has at most 256"),
    ([(A.LOAD, R.XCONST, 0, 0), (A.EMIT, 0, 0, 0)], dict(log2_trace=7), "trace 2^7, LDE 2^6"),
]


@pytest.mark.parametrize("field", FIELDS)
def test_every_refusal_of_the_rap_check(exe, field):
    for ops, kw, message in REFUSALS:
        assert check_program(exe, field, ops, **kw) == ["fail", message], message


def typed_cases():
    from lambda_elliptic_curves_amd import stark
    S = stark
    every_pair = []
    for k, op in enumerate(("add", "sub", "mul")):
        f, e = S.cell(0, k), S.xcell(0, k)
        ff, fe, ef, ee = f._bin(op, S.cell(1)), f._bin(op, S.xconst(0)), e._bin(op, S.cell(1)), e._bin(op, S.xconst(1))
        every_pair += [ff, fe, ef, ee, -ff, -ee]
    eight = S.xcell(0, 8)
    for k in reversed(range(8)):
        eight = eight * (S.xcell(0, k) + S.cell(1, k))
    yield "every pair", stark.compile_transitions(every_pair).ops.tolist(), len(every_pair)
    yield "eight in E", stark.compile_transitions([eight]).ops.tolist(), 1
    yield "rom", stark.compile_transitions(R.RAP_AIRS["rom"][0](stark)).ops.tolist(), 3
    yield "all in F", stark.compile_transitions(A.AIRS["rom"][0](stark)).ops.tolist(), 3
    yield "F then E in one slot", [(A.LOAD, A.CELL, 0, 0), (A.STORE, 0, 1, 0), (A.LOAD, A.TMP, 1, 0), (A.MUL, R.XCONST, 0, 0), (A.STORE, 0, 1, 0),
                                   (A.LOAD, A.CELL, 1, 0), (A.STORE, 0, 3, 0), (A.SUB, A.TMP, 1, 0), (A.EMIT, 0, 0, 0), (A.LOAD, A.TMP, 3, 0),
                                   (A.EMIT, 0, 1, 0)], 2
    yield "empty", [], 0


@pytest.mark.parametrize("field", FIELDS)
def test_typing_against_the_model(exe, field):
    F = M.FIELDS[field]
    for name, ops, n_transitions in typed_cases():
        words, n_tmps, n_ext, slots = R.type_program(ops, F.width)
        got = check_program(exe, field, ops, n_consts=3, n_xconsts=2, n_cols=5, n_xcols=1, n_transitions=n_transitions)
        assert got[0] == f"ok {n_tmps} {n_ext} {slots}", name
        assert [int(w) for w in got[1].split()] == words, name
        if name == "eight in E":
            assert (n_tmps, n_ext, slots) == (8, 8, 8 * F.width)
        if name == "F then E in one slot":   # the model itself, by hand: tmp 1 first a word, then an element; tmp 3 a word; tmp 0, 2 unused
            assert (n_tmps, n_ext, slots) == (4, 1, 3 + F.width)
            #                                LOAD STORE LOAD MUL STORE LOAD STORE SUB EMIT LOAD EMIT   (bit 0: the accumulator is in E, bit 1: the operand)
            assert [(w >> 4) & 3 for w in words] == [0, 0, 0, 2, 1, 0, 0, 2, 1, 0, 0]
            assert [(w >> 16) & 0xffff for w in words][1:8:3] == [1, 1, 1] and (words[6] >> 16) & 0xffff == 2 + F.width   # tmp 1 at slot 1, tmp 3 after its D slots and tmp 2
        if name == "all in F":   # nothing is typed: the words are the plain op words
            assert words == [op | src << 8 | index << 16 | row << 32 for op, src, index, row in ops]


@pytest.mark.parametrize("field", FIELDS)
def test_coefficient_tables_under_sanitizers(exe, field):
    F = M.FIELDS[field]
    rng = np.random.default_rng(5)
    elem = lambda: tuple(int.from_bytes(rng.bytes(16), "big") % F.p for _ in range(F.width))
    for n_num, n_den in ((16, 16), (0, 1), (3, 0), (0, 0)):
        sides = [[(int(rng.integers(0, 5)), elem()) for _ in range(k)] for k in (n_num, n_den)]
        sides[-1][:1] = [(4, (F.p - 1,) * F.width)][:len(sides[-1])]
        words = [5]
        for side in sides:
            words.append(len(side))
            for col, coeff in side:
                words += [col] + list(F.word_elem(coeff))
        got = [tuple(int(w) for w in line.split()) for line in host(exe, field, "terms", words)]
        assert got == [(4096 * (col + 1), 0) + F.word_elem(coeff) for side in sides for col, coeff in side]


@pytest.mark.parametrize("field", FIELDS)
def test_step_groups_with_values_in_the_extension(exe, field):
    F, E = M.FIELDS[field], M.FIELDS[field].ext
    log2_trace = 5
    n, g = 1 << log2_trace, F.root(log2_trace)
    rng = np.random.default_rng(6)
    elem = lambda: tuple(int.from_bytes(rng.bytes(16), "big") % F.p for _ in range(F.width))
    boundary = [(k % 3, k % 2, step, elem() if k % 3 else M.lift(F, 7 + k), elem()) for k, step in enumerate([5, 0, n - 1, 5, n + 5, 2, 0, 2 * n])]
    boundary.append((0, 1, 9, (F.p - 1,) * F.width, (F.p - 1,) * F.width))
    for bnd in (boundary, boundary[:1], []):
        words = [log2_trace, F.word(g), len(bnd)]
        for col, is_aux, step, value, coeff in bnd:
            words += [col, is_aux, step] + list(F.word_elem(value)) + list(F.word_elem(coeff))
        got = [tuple(int(w) for w in line.split()) for line in host(exe, field, "steps", words)]
        order = sorted(range(len(bnd)), key=lambda k: bnd[k][2] % n)
        want, q = [tuple(order)], 0
        while q < len(order):
            step = bnd[order[q]][2] % n
            group = [k for k in order[q:] if bnd[k][2] % n == step]
            const = F.zero
            for k in group:
                const = E.add(const, E.mul(bnd[k][4], bnd[k][3]))
            want += [(F.word(pow(g, step, F.p)), q, len(group)), F.word_elem(const)]
            q += len(group)
        assert got == want
