"""Round 2 over Goldilocks with Fp2 and BabyBear with Fp4 without a device: every status the two constraint-evaluation and
the two parts entry points return before any device work (which pins the order of their checks), the model of
tests/ext_round2_ref.py against stark_round2_ref where the coefficients lie in F, and the host tables of
csrc/ext_round2.cuh (descriptor classes, step groups, combined constants) compiled for the host with the address and
undefined-behaviour sanitizers (tests/ext_round2_host_main.cpp), run as a child process and compared with Python."""
import os
import subprocess

import numpy as np
import pytest

from tests import air_program_ref as A
from tests import ext_round2_ref as M
from tests import stark_round2_ref as R2

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ["gl2", "bb4"]
NP = {"gl2": np.uint64, "bb4": np.uint32}
BAD_ARG, INV_ZERO = r"\[-9\]", r"\[-10\]"


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


def fib_program():
    from lambda_elliptic_curves_amd import stark
    return stark.compile_transitions(A.AIRS["fib2"][0](stark))


def call(name, program=None, consts=(), n_cols=2, log2_trace=4, log2_blowup=2, boundary=None, transitions=None, offset=3, out=None, cols=None):
    F = M.FIELDS[name]
    N = 1 << min(log2_trace + log2_blowup, 10)   # the buffers are never read: the checks come first
    one = F.word_elem(M.lift(F, 1))
    if boundary is None:
        boundary = [(0, 0, F.word(1), one)]
    if transitions is None:
        transitions = [dict(period=1, offset=0, end_exemptions=1, coeff=one)] * 2
    cols = cols if cols is not None else [Buffer(name, N) for _ in range(n_cols)]
    out = out or Buffer(name, F.width * N)
    off = None if offset is None else F.word(offset) if name == "bb4" or offset < F.p else offset
    return module(name).constraint_evaluations_device(program or fib_program(), list(consts), cols, log2_trace, log2_blowup, boundary, transitions, t_out=out,
                                                      offset=off, stream=0)


def refused(code, text=None):
    from lambda_elliptic_curves_amd import errors
    kind = errors.FieldError if code == INV_ZERO else errors.HipError
    return pytest.raises(kind, match=code + (".*" + text if text else ""))


@pytest.mark.parametrize("field", FIELDS)
def test_constraint_evaluations_argument_rules(field):
    F = M.FIELDS[field]
    one = F.word_elem(M.lift(F, 1))
    tr = lambda **kw: [dict(dict(period=1, offset=0, end_exemptions=1, coeff=one), **kw)] * 2
    with refused(BAD_ARG, "period 0"):
        call(field, transitions=tr(period=0))
    with refused(BAD_ARG, "exceed the trace"):
        call(field, transitions=tr(period=4, end_exemptions=5))       # 20 > n = 16
    call_ok_shape = tr(period=4, end_exemptions=4)                    # 16 = n is legal: only later checks can refuse it
    with refused(INV_ZERO):
        call(field, transitions=call_ok_shape, offset=1)
    with refused(BAD_ARG, "column 2 of 2"):
        call(field, boundary=[(2, 0, F.word(1), one)])
    too_large = {"gl2": (29, 2), "bb4": (23, 2)}[field]
    with refused(BAD_ARG, "beyond the transform"):
        call(field, log2_trace=too_large[0], log2_blowup=too_large[1])
    with refused(BAD_ARG, "16-byte aligned"):
        call(field, out=Buffer(field, F.width * 64, skew=1))
    with refused(BAD_ARG, "column 1: null or misaligned"):
        call(field, cols=[Buffer(field, 64), Buffer(field, 64, skew=1)])
    shared = Buffer(field, F.width * 64)
    with refused(BAD_ARG, "out overlaps column 1"):
        call(field, out=shared, cols=[Buffer(field, 64), shared])
    with refused(BAD_ARG, "distinct transition zerofiers"):
        from lambda_elliptic_curves_amd import stark
        nine = stark.compile_transitions([stark.cell(0, 1 + k % 3) - stark.cell(0) for k in range(9)])
        call(field, program=nine, transitions=[dict(period=1, offset=k, end_exemptions=0, coeff=one) for k in range(9)])


@pytest.mark.parametrize("field", FIELDS)
def test_zero_denominators_are_refused_on_the_host(field):
    F = M.FIELDS[field]
    for offset in (None, 1, F.root(6), F.p - 1):          # h^N = 1, a NULL offset included (N = 64)
        with refused(INV_ZERO, "h\\^N = 1"):
            call(field, offset=offset)
        with refused(INV_ZERO, "h\\^N = 1"):
            call(field, boundary=[], offset=offset)         # transitions alone
    with refused(INV_ZERO, "offset is zero"):
        call(field, offset=0)
    if field == "gl2":
        with refused(INV_ZERO, "offset is zero"):
            call(field, offset=F.p)                         # any u64 is a word: p is zero


def test_babybear_words_must_be_below_p():
    F, p = M.BB4, M.BB4.p
    one = F.word_elem(M.lift(F, 1))
    from lambda_elliptic_curves_amd import stark
    with_const = stark.compile_transitions([stark.cell(0, 1) - stark.const(0) * stark.cell(1), stark.cell(1, 1) - stark.cell(0)])
    with refused(BAD_ARG, "constants: word 0"):
        module("bb4").constraint_evaluations_device(with_const, [p], [Buffer("bb4", 64), Buffer("bb4", 64)], 4, 2, [], [dict(coeff=one)] * 2,
                                                    t_out=Buffer("bb4", 256), offset=3, stream=0)
    with refused(BAD_ARG, "transition coefficient"):
        call("bb4", transitions=[dict(period=1, coeff=(0, 0, p, 0))] * 2)
    with refused(BAD_ARG, "boundary coefficient"):
        call("bb4", boundary=[(0, 0, 1, (0, 0, 0, p))])
    with refused(BAD_ARG, "boundary value"):
        call("bb4", boundary=[(0, 0, p, one)])
    with refused(BAD_ARG, "offset is not below p"):
        module("bb4").constraint_evaluations_device(fib_program(), [], [Buffer("bb4", 64), Buffer("bb4", 64)], 4, 2, [], [dict(coeff=one)] * 2,
                                                    t_out=Buffer("bb4", 256), offset=p, stream=0)


@pytest.mark.parametrize("field", FIELDS)
def test_a_malformed_program_is_refused_with_the_op_named(field):
    from lambda_elliptic_curves_amd import stark
    bad = stark.AirProgram(np.array([(A.LOAD, A.CELL, 0, 0), (A.ADD, A.TMP, 3, 0), (A.EMIT, 0, 0, 0), (A.EMIT, 0, 1, 0)], dtype=stark.AIR_OP_DTYPE), 2)
    with refused(BAD_ARG, "AIR program: op 1: temporary 3 is read before it is stored"):
        call(field, program=bad)
    # the order of the checks: the program before the coefficients' classes, the buffers and the offset
    with refused(BAD_ARG, "AIR program: op 1"):
        call(field, program=bad, offset=1, out=Buffer(field, 256, skew=1))
    # ... the domain before the program, the tables before the buffers, the buffers before the offset
    with refused(BAD_ARG, "beyond the transform"):
        call(field, program=bad, log2_trace=40)
    F = M.FIELDS[field]
    with refused(BAD_ARG, "period 0"):
        call(field, transitions=[dict(period=0, coeff=F.word_elem(M.lift(F, 1)))] * 2, out=Buffer(field, 256, skew=1))
    with refused(BAD_ARG, "16-byte aligned"):
        call(field, offset=1, out=Buffer(field, 256, skew=1))
    short = stark.compile_transitions(A.AIRS["periodic"][0](stark))
    with refused(BAD_ARG, "short one"):
        module(field).constraint_evaluations_device(short, [], [Buffer(field, 64), Buffer(field, 8)], 4, 2, [(1, 0, 0, F.word_elem(M.lift(F, 1)))],
                                                    [dict(coeff=F.word_elem(M.lift(F, 1)))], t_out=Buffer(field, 256), offset=3, col_log2_len=[6, 3], stream=0)


@pytest.mark.parametrize("field", FIELDS)
def test_composition_parts_argument_rules(field):
    F = M.FIELDS[field]
    X = module(field)

    def parts(n_parts, log2_lde=6, offset=3, skew=0):
        import torch
        # t_evals only hands its pointer on; the outputs are torch's own (host) tensors, never written
        ev = torch.zeros(F.width * 64 + 4, dtype=torch.int64 if field == "gl2" else torch.int32)
        return X.composition_parts_device(ev[skew:], log2_lde, n_parts, offset=None if offset is None else offset, stream=0)

    with refused(BAD_ARG, "0 parts"):
        parts(0)
    with refused(BAD_ARG, "65 parts"):
        parts(65)
    from lambda_elliptic_curves_amd import _lib, errors
    with refused(BAD_ARG, "beyond the transform"):   # the C call itself: the wrapper would allocate the outputs of such a domain first
        tail = [1, None, None, None, None]
        errors.check(_lib.lib().lw_goldilocks_ext2_composition_parts_device(None, 0, 31, None, 0, *tail) if field == "gl2" else
                     _lib.lib().lw_babybear_ext4_composition_parts_device(None, 0, 25, None, *tail))
    with refused(BAD_ARG, "16-byte aligned"):
        parts(2, skew=1)
    with refused(INV_ZERO, "offset is zero"):
        parts(2, offset=0)


def test_model_with_base_field_coefficients_is_the_256_bit_model():
    """ext_round2_ref with every coefficient in F against stark_round2_ref.evaluate at p = BabyBear"""
    F = M.BB4
    from lambda_elliptic_curves_amd import stark
    for name in ("fib2", "rom", "periodic"):
        build, n_cols, n_consts, periodic = A.AIRS[name]
        dom, ref_dom = M.domain(F, 3, 2, 3), R2.Domain(F.p, 3, 2, 3)
        assert (dom.g, dom.w) == (ref_dom.g, ref_dom.w)
        cols = [A.fill(F.p, periodic[c] * dom.blowup if c in periodic else dom.N, 5 + c) for c in range(n_cols)]
        consts = A.fill(F.p, n_consts, 9)
        program = stark.compile_transitions(build(stark))
        coeffs = A.fill(F.p, program.n_transitions + 2, 10)
        transitions = [dict(period=1 + c % 2, offset=c % 2, end_exemptions=c % 3, coeff=coeffs[c]) for c in range(program.n_transitions)]
        boundary = [(0, 0, 4, coeffs[-1]), (0, dom.n - 1, 6, coeffs[-2])]
        want = R2.evaluate(ref_dom, cols, boundary, transitions, A.run_all(program.ops.tolist(), ref_dom, cols, consts, program.n_transitions))
        got = M.evaluate(F, dom, cols, program.ops.tolist(), consts, [(c, s, v, M.lift(F, k)) for c, s, v, k in boundary],
                         [dict(t, coeff=M.lift(F, t["coeff"])) for t in transitions])
        assert got == [M.lift(F, v) for v in want]


# ---- the host tables under the sanitizers
@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    hipcc = "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        hipcc = "hipcc"
    out = tmp_path_factory.mktemp("ext_round2") / "ext_round2_host"
    subprocess.check_call([hipcc, "-x", "hip", "--cuda-host-only", "-O2", "-std=c++17", "-Xarch_host", "-fsanitize=address,undefined",
                           "-Xarch_host", "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "lambda_elliptic_curves_amd", "csrc"),
                           os.path.join(ROOT, "tests", "ext_round2_host_main.cpp"), "-o", str(out)], timeout=600)
    return str(out)


def expected_tables(F, log2_trace, log2_blowup, transitions, boundary):
    """canonical tables -> the printed lines, words as the library stores them"""
    E, p, n, N = F.ext, F.p, 1 << log2_trace, 1 << (log2_trace + log2_blowup)
    g = F.root(log2_trace)
    keys, lines = [], []
    for t in transitions:
        if t[:5] not in keys:
            keys.append(t[:5])
    lines.append(tuple(keys.index(t[:5]) for t in transitions))
    for period, offset, ee, ep, peo in keys:
        lines.append((min((1 << log2_blowup) * (ep or period), N), n // period, n // ep if ep else 0, F.word(pow(g, offset * n // period % n, p)),
                      F.word(pow(g, n * peo // ep % n, p) if ep else 1), 1 if ep else 0))
        lines.append(tuple(F.word(pow(g, (n - k * period) % n, p)) for k in range(1, ee + 1)))
    order = sorted(range(len(boundary)), key=lambda k: boundary[k][1] % n)   # stable
    lines.append(tuple(order))
    q = 0
    while q < len(order):
        step = boundary[order[q]][1] % n
        group = [k for k in order[q:] if boundary[k][1] % n == step]
        const = F.zero
        for k in group:
            const = E.add(const, E.mul_base(boundary[k][3], boundary[k][2]))
        lines.append((F.word(pow(g, step, p)), q, len(group)))
        lines.append(F.word_elem(const))
        q += len(group)
    return lines


@pytest.mark.parametrize("field", FIELDS)
def test_host_tables_under_sanitizers(exe, field):
    F = M.FIELDS[field]
    log2_trace, log2_blowup = 5, 2
    n = 1 << log2_trace
    rng = np.random.default_rng(7)
    elem = lambda: tuple(int.from_bytes(rng.bytes(16), "big") % F.p for _ in range(F.width))
    descs = [(1, 0, 1, 0, 0), (2, 1, 2, 0, 0), (1, 0, 1, 0, 0), (2, 1, 1, 4, 1), (3, 2, 3, 5, 2), (2, 1, 2, 0, 0), (1, 0, 0, 0, 0), (n, n - 1, 1, 0, 0),
             (64, 1, 0, 0, 0)]
    transitions = [d + (elem(),) for d in descs]
    boundary = [(k % 3, step, int.from_bytes(rng.bytes(16), "big") % F.p, elem()) for k, step in enumerate([5, 0, n - 1, 5, n + 5, 2, 0, 2 * n])]
    boundary.append((0, 9, F.p - 1, (F.p - 1,) * F.width))
    for trs, bnd in ((transitions, boundary), ([], boundary[:1]), (transitions[:1], [])):
        words = [log2_trace, log2_blowup, F.word(F.root(log2_trace)), len(trs)]
        for t in trs:
            words += list(t[:5]) + list(F.word_elem(t[5]))
        words.append(len(bnd))
        for col, step, value, coeff in bnd:
            words += [col, step, F.word(value)] + list(F.word_elem(coeff))
        out = subprocess.run([exe, field] + [str(w) for w in words], capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, out.stderr[-2000:]
        got = [tuple(int(w) for w in line.split()) for line in out.stdout.splitlines()]
        assert got == expected_tables(F, log2_trace, log2_blowup, trs, bnd)
