"""Circle STARK round 2 over Mersenne31 without a device: the properties the model of tests/circle_round2_ref.py rests on
(zero sets and cycle lengths of the zerofiers, no zero on the LDE coset, the block split of the parts, the low degree of the
quotients exactly for a valid trace), every status the two entry points return before any device work, which pins the order
of their checks, and the host tables of csrc/circle_round2.cuh compiled for the host with the address and undefined-behaviour
sanitizers (tests/circle_round2_host_main.cpp), run as a child process and compared with Python."""
import os
import random
import subprocess

import numpy as np
import pytest

from tests import air_program_ref as A
from tests import circle_ref as CR
from tests import circle_round2_ref as M
from tests import mersenne31_ext_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = M.P
BAD_ARG, INV_ZERO = r"\[-9\]", r"\[-10\]"
ONE = (1, 0, 0, 0)
DESCRIPTORS = [dict(period=1, offset=0, end_exemptions=0), dict(period=1, offset=0, end_exemptions=2), dict(period=2, offset=1, end_exemptions=1),
               dict(period=4, offset=3, end_exemptions=4), dict(period=8, offset=5, end_exemptions=1)]


def rand_elems(n, seed):
    rnd = random.Random(seed)
    return [tuple(rnd.randrange(P) for _ in range(4)) for _ in range(n)]


def stark():
    from lambda_elliptic_curves_amd import stark as S
    return S


def quadratic_case(dom, broken=False):
    """a trace a' = a^2 of n rows, its LDE, the program, one end exemption, one boundary constraint"""
    a = [3]
    for _ in range(dom.n - 1):
        a.append(a[-1] * a[-1] % P)
    if broken:
        a[5] = (a[5] + 1) % P
    lde = CR.evaluate_cfft(CR.interpolate_cfft(a) + [0] * (dom.N - dom.n))
    program = stark().compile_transitions(A.AIRS["quadratic"][0](stark()))
    beta, gamma = rand_elems(2, 7)
    return a, [lde], program, [(0, 0, 3, gamma)], [dict(period=1, offset=0, end_exemptions=1, coeff=beta)]


# ---- the model
@pytest.mark.parametrize("t", DESCRIPTORS, ids=lambda t: "period%d_offset%d_ex%d" % (t["period"], t["offset"], t["end_exemptions"]))
def test_zerofier_zero_sets_cycle_lengths_and_no_zero_on_the_lde_coset(t):
    dom = M.Domain(4, 2)
    on_trace = [M.zerofier(dom, t, q) for q in dom.trace_points]
    assert [j for j, z in enumerate(on_trace) if z == 0] == list(range(t["offset"], dom.n, t["period"]))
    # E vanishes exactly at the exempted rows, so E / Z has its zeros' poles at constrained_rows only
    ex = [M.exemptions(dom, t, q) for q in dom.trace_points]
    exempt = [j for j, e in enumerate(ex) if e == 0]
    assert sorted(exempt + M.constrained_rows(dom, t)) == list(range(t["offset"], dom.n, t["period"]))
    assert [dom.trace_points[j] for j in exempt[::-1]] == M.exemption_points(dom, t)
    on_lde = [M.zerofier(dom, t, q) for q in dom.lde_points]
    assert 0 not in on_lde and 0 not in [M.exemptions(dom, t, q) for q in dom.lde_points]
    cycle = 2 * dom.blowup * t["period"]
    assert cycle <= dom.N and on_lde == (on_lde[:cycle] * (dom.N // cycle))
    assert cycle == 2 or on_lde[: cycle // 2] != on_lde[cycle // 2: cycle]       # no shorter cycle
    # the simple zero: Z is a polynomial of total degree m / 2, so it has m zeros on the circle and they are these
    assert len([z for z in on_trace if z == 0]) == dom.n // t["period"]


def test_lde_rows_step_by_the_blowup_and_the_boundary_denominator_never_vanishes():
    dom = M.Domain(3, 2)
    g = CR.subgroup_generator(dom.log2_trace)
    for i, q in enumerate(dom.lde_points):
        assert CR.padd(q, g) == dom.lde_points[(i + dom.blowup) % dom.N]
        assert M.psub(CR.padd(q, g), g) == q
    for step in range(dom.n):
        ys = [M.psub(q, dom.trace_points[step])[1] for q in dom.lde_points]
        assert 0 not in ys
        zeros = [j for j, p in enumerate(dom.trace_points) if M.psub(p, dom.trace_points[step])[1] == 0]
        assert zeros == sorted([step, (step + dom.n // 2) % dom.n])                   # the point and its antipode


def test_block_split_identity_and_part_factors():
    from lambda_elliptic_curves_amd import mersenne31_ext as E
    rnd = random.Random(3)
    c = [rnd.randrange(P) for _ in range(64)]
    z = R.circle_point(rand_elems(1, 4)[0])
    for log2_part, n_parts in ((6, 1), (5, 2), (4, 4), (3, 8), (1, 32), (3, 4)):
        L = 1 << log2_part
        f = M.part_factors(z, log2_part, n_parts)
        assert E.part_factors(z, log2_part, n_parts) == f and f[0] == R.ONE
        total = R.ZERO
        for j in range(n_parts):
            total = R.add(total, R.mul(f[j], R.evaluate(c[j * L:(j + 1) * L], z)))
        assert total == R.evaluate(c[: n_parts * L], z)
    with pytest.raises(Exception):
        E.part_factors(z, 0, 2)
    with pytest.raises(Exception):
        E.part_factors(z, 3, 3)
    assert E.part_factors(((P, 1 << 31, 0, 1), ONE), 2, 2) == M.part_factors((R.elem((P, 1 << 31, 0, 1)), ONE), 2, 2)   # any u32 is a word


def test_low_degree_exactly_for_a_valid_trace_at_n_16():
    dom = M.Domain(4, 2)
    bound = M.degree_bound(dom, 2, 1)
    assert bound == 32
    a, cols, program, boundary, transitions = quadratic_case(dom)
    ev = M.evaluate(dom, cols, program.ops.tolist(), [], boundary, transitions)
    assert M.last_nonzero(ev) == 18 < bound
    coeffs, lde, tail = M.parts(dom, ev, 4, 2)
    assert tail == 0 and len(coeffs) == 8 and all(len(c) == 16 for c in coeffs) and all(len(v) == dom.N for v in lde)
    # every part's LDE plane is the part's polynomial on the coset, and the parts rebuild the evaluations
    for i, q in enumerate(dom.lde_points):
        f = M.part_factors(M.lift(q), 4, 2)
        total = R.ZERO
        for j in range(2):
            total = R.add(total, R.mul(f[j], tuple(lde[4 * j + e][i] for e in range(4))))
        assert total == ev[i]
    _, cols, _, _, _ = quadratic_case(dom, broken=True)
    bad = M.evaluate(dom, cols, program.ops.tolist(), [], boundary, transitions)
    assert M.last_nonzero(bad) == 63
    assert M.parts(dom, bad, 4, 2)[2] > 0
    # a wrong boundary value alone breaks it too
    wrong = M.evaluate(dom, quadratic_case(dom)[1], program.ops.tolist(), [], [(0, 0, 4, boundary[0][3])], transitions)
    assert M.last_nonzero(wrong) >= bound


def test_the_identity_at_a_point_of_the_circle_over_qm31():
    """the formulas over QM31 are those over F_p: at a lifted LDE point composition_at gives the evaluation there"""
    dom = M.Domain(3, 2)
    a, cols, program, boundary, transitions = quadratic_case(dom)
    ev = M.evaluate(dom, cols, program.ops.tolist(), [], boundary, transitions)
    for i in (0, 5, dom.N - 1):
        cell = lambda col, row, i=i: R.embed(cols[col][(i + row * dom.blowup) % dom.N])
        assert M.composition_at(dom, cell, program.ops.tolist(), [], boundary, transitions, M.lift(dom.lde_points[i])) == ev[i]
        assert M.frame_points(dom, M.lift(dom.lde_points[i]), [1])[0] == M.lift(dom.lde_points[(i + dom.blowup) % dom.N])
    # a periodic column of period 2 read at (n / 2) q_i: the coset of 2 B points, index i mod 2 B
    for i in (1, 9, 30):
        assert M.periodic_point(dom, 2, M.lift(dom.lde_points[i])) == M.lift(CR.coset_points(3)[i % 8])


# ---- every status, before any device work
class Buffer:
    """host memory where the calls expect device memory: the checks under test never follow a pointer"""

    def __init__(self, n_words, skew=0):
        self.a = np.zeros(n_words + 4, np.uint32)
        self.skew = skew
        self.device = "cpu"

    def data_ptr(self):
        return self.a.ctypes.data + 4 * self.skew


def fib_program():
    return stark().compile_transitions(A.AIRS["fib2"][0](stark()))


def call(program=None, consts=(), n_cols=2, log2_trace=4, log2_blowup=2, boundary=None, transitions=None, out=None, cols=None, lens=None):
    from lambda_elliptic_curves_amd import mersenne31_ext as E
    N = 1 << min(log2_trace + log2_blowup, 10)   # the buffers are never read: the checks come first
    if boundary is None:
        boundary = [(0, 0, 1, ONE)]
    if transitions is None:
        transitions = [dict(period=1, offset=0, end_exemptions=1, coeff=ONE)] * 2
    cols = cols if cols is not None else [Buffer(N) for _ in range(n_cols)]
    return E.constraint_evaluations_device(program if program is not None else fib_program(), list(consts), cols, log2_trace, log2_blowup, boundary, transitions,
                                           t_out=out or Buffer(4 * N), col_log2_len=lens, stream=0)


def refused(code, text=None):
    from lambda_elliptic_curves_amd import errors
    kind = errors.FieldError if code == INV_ZERO else errors.HipError
    return pytest.raises(kind, match=code + (".*" + text if text else ""))


def test_constraint_evaluations_statuses():
    tr = lambda **kw: [dict(dict(period=1, offset=0, end_exemptions=1, coeff=ONE), **kw)] * 2
    with refused(BAD_ARG, "at least 2 rows"):
        call(log2_trace=0)
    with refused(BAD_ARG, "at most 2\\^30"):
        call(log2_trace=29, log2_blowup=2)
    for period in (0, 3, 16, 32):                                       # n = 16: 8 is the largest
        with refused(BAD_ARG, "period %d is not a power of two" % period):
            call(transitions=tr(period=period))
    with refused(BAD_ARG, "offset 2 of period 2"):
        call(transitions=tr(period=2, offset=2))
    with refused(BAD_ARG, "exceed the trace"):
        call(transitions=tr(period=4, end_exemptions=5))
    with refused(BAD_ARG, "column 2 of 2"):
        call(boundary=[(2, 0, 1, ONE)])
    with refused(BAD_ARG, "step 16 of a trace of 16"):
        call(boundary=[(0, 16, 1, ONE)])
    short = stark().compile_transitions(A.AIRS["periodic"][0](stark()))
    with refused(BAD_ARG, "short one"):
        call(program=short, cols=[Buffer(64), Buffer(8)], lens=[6, 3], boundary=[(1, 0, 0, ONE)], transitions=tr()[:1])
    nine = stark().compile_transitions([stark().cell(0, 1 + k % 3) - stark().cell(0) for k in range(9)])
    with refused(BAD_ARG, "9 distinct transition zerofiers"):
        call(program=nine, transitions=[dict(period=1, offset=0, end_exemptions=k, coeff=ONE) for k in range(9)])
    bad = stark().AirProgram(np.array([(A.LOAD, A.CELL, 0, 0), (A.ADD, A.TMP, 3, 0), (A.EMIT, 0, 0, 0), (A.EMIT, 0, 1, 0)], dtype=stark().AIR_OP_DTYPE), 2)
    with refused(BAD_ARG, "AIR program: op 1: temporary 3 is read before it is stored"):
        call(program=bad)
    with refused(BAD_ARG, "16-byte aligned"):
        call(out=Buffer(256, skew=1))
    with refused(BAD_ARG, "column 1: null or misaligned"):
        call(cols=[Buffer(64), Buffer(64, skew=1)])
    shared = Buffer(256)
    with refused(BAD_ARG, "out overlaps column 1"):
        call(out=shared, cols=[Buffer(64), shared])
    with refused(INV_ZERO, "blow-up of 1"):
        call(log2_blowup=0)
    with refused(INV_ZERO, "blow-up of 1"):
        call(log2_blowup=0, boundary=[])
    with refused(INV_ZERO, "blow-up of 1"):
        call(log2_blowup=0, program=stark().AirProgram(np.zeros(0, stark().AIR_OP_DTYPE), 0), transitions=[])
    # legal shapes get past every check: without a device the next status is the missing device's, with one the call runs on
    # host memory, so only the refusals are asked for here; the last legal descriptors are the GPU tests' business


def test_the_order_of_the_checks():
    bad = stark().AirProgram(np.array([(A.LOAD, A.CELL, 0, 0), (A.ADD, A.TMP, 3, 0), (A.EMIT, 0, 0, 0), (A.EMIT, 0, 1, 0)], dtype=stark().AIR_OP_DTYPE), 2)
    tr = lambda **kw: [dict(dict(period=1, offset=0, end_exemptions=1, coeff=ONE), **kw)] * 2
    with refused(BAD_ARG, "at least 2 rows"):                             # the domain before the program
        call(program=bad, log2_trace=0)
    with refused(BAD_ARG, "AIR program: op 1"):                           # the program before the entries and the buffers
        call(program=bad, boundary=[(2, 0, 1, ONE)], out=Buffer(256, skew=1))
    with refused(BAD_ARG, "column 2 of 2"):                               # the boundary entries before the transitions
        call(boundary=[(2, 0, 1, ONE)], transitions=tr(period=0))
    with refused(BAD_ARG, "period 0"):                                    # the transitions before the buffers
        call(transitions=tr(period=0), out=Buffer(256, skew=1))
    with refused(BAD_ARG, "16-byte aligned"):                             # the buffers before the blow-up
        call(log2_blowup=0, out=Buffer(64, skew=1))
    with refused(BAD_ARG, "exceed the trace"):                            # ... which comes last
        call(log2_blowup=0, transitions=tr(period=4, end_exemptions=5))


def test_composition_parts_statuses():
    import torch
    from lambda_elliptic_curves_amd import mersenne31_ext as E

    def parts(log2_part, n_parts, log2_lde=6, skew=0, lde=True):
        ev = torch.zeros(4 * 64 + 4, dtype=torch.int32)   # hands its pointer on; the outputs are torch's own (host) tensors, never written
        return E.composition_parts_device(ev[skew:], log2_lde, log2_part, n_parts, lde=lde, stream=0)

    for log2_part, n_parts in ((3, 0), (3, 3), (0, 4), (4, 8), (6, 2)):
        with refused(BAD_ARG, "a power of two of parts"):
            parts(log2_part, n_parts)
    with refused(BAD_ARG, "at least 2 points"):
        parts(1, 1, log2_lde=0)
    from lambda_elliptic_curves_amd import errors
    with pytest.raises(errors.OrderError):
        parts(3, 2, log2_lde=31, lde=False)
    with refused(BAD_ARG, "16-byte aligned"):
        parts(3, 2, skew=1)
    ev = torch.zeros(4 * 64 + 4, dtype=torch.int32)
    from lambda_elliptic_curves_amd import _lib as L
    import ctypes as C
    at = lambda w: C.c_void_p(ev.data_ptr() + 4 * w)
    f = L.lib().lw_mersenne31_ext4_composition_parts_device
    big = torch.zeros(4 * 64 * 4 + 64, dtype=torch.int32)
    to = lambda w: C.c_void_p(big.data_ptr() + 4 * w)
    assert f(at(0), 0, 4, 2, 2, at(32), None, None, None) == L.ERR_BAD_ARG             # coefficients inside the evaluations
    assert f(at(0), 0, 4, 2, 2, to(0), at(16), None, None) == L.ERR_BAD_ARG            # the LDE planes inside the evaluations
    assert f(at(0), 0, 4, 2, 2, to(0), to(16), None, None) == L.ERR_BAD_ARG            # the LDE planes inside the coefficients
    assert f(at(0), 8, 4, 2, 2, to(0), None, None, None) == L.ERR_BAD_ARG              # a stride below the length
    assert f(None, 0, 4, 2, 2, to(0), None, None, None) == L.ERR_BAD_ARG
    assert f(at(0), 0, 4, 2, 2, None, None, None, None) == L.ERR_BAD_ARG
    assert not ev.any() and not big.any()


def test_symbols_structs_and_wrappers():
    import ctypes as C
    from lambda_elliptic_curves_amd import _lib
    from lambda_elliptic_curves_amd import mersenne31_ext as E
    header = open(os.path.join(ROOT, "include", "lw_hip.h")).read()
    ffi = open(os.path.join(ROOT, "rust-shim", "src", "ffi.rs")).read()
    for sym in ("lw_mersenne31_ext4_constraint_evaluations_device", "lw_mersenne31_ext4_composition_parts_device"):
        assert sym in _lib.EXPORTS and hasattr(_lib.lib(), sym)
        assert "int %s(" % sym in header and "pub fn %s(" % sym in ffi
    assert C.sizeof(_lib.M31qBoundary) == 40 and C.sizeof(_lib.M31qTransition) == 40
    assert "} lw_m31q_boundary_t;" in header and "} lw_m31q_transition_t;" in header
    assert "d n / 2 + 2 e - m / 2" in header and "smallest power of two greater than 2 D" in header   # the degree to budget
    for name in ("constraint_evaluations_device", "composition_parts_device", "round2_device", "part_factors"):
        assert callable(getattr(E, name))
    with pytest.raises(ValueError):
        call(transitions=[dict(period=1, offset=0, end_exemptions=0, exemptions_period=2, coeff=ONE)] * 2)


# ---- the host tables, sanitised, as a child process
def test_host_program_of_the_tables(tmp_path):
    hipcc = "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        hipcc = "hipcc"
    exe = tmp_path / "circle_round2_host"
    subprocess.check_call([hipcc, "-x", "hip", "--cuda-host-only", "-O2", "-std=c++17", "-Xarch_host", "-fsanitize=address,undefined",
                           "-Xarch_host", "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "lambda_elliptic_curves_amd", "csrc"),
                           os.path.join(ROOT, "tests", "circle_round2_host_main.cpp"), "-o", str(exe)], timeout=600)
    log2_trace, log2_blowup = 5, 2
    dom = M.Domain(log2_trace, log2_blowup)
    trs = [dict(period=1, offset=0, end_exemptions=2), dict(period=2, offset=1, end_exemptions=1), dict(period=1, offset=0, end_exemptions=2),
           dict(period=16, offset=9, end_exemptions=2), dict(period=1, offset=0, end_exemptions=0), dict(period=2, offset=1, end_exemptions=1),
           dict(period=4, offset=0, end_exemptions=8)]
    g = rand_elems(7, 21)
    edge = (P, 1 << 31, (1 << 32) - 1, P - 1)
    bnd = [(0, 5, 9, g[0]), (1, 0, (1 << 32) - 1, g[1]), (0, 31, P, edge), (2, 5, 1 << 31, g[3]), (1, 17, 0, g[4]), (0, 0, 3, g[5]), (2, 5, 1, g[6])]
    args = [log2_trace, log2_blowup, len(trs)] + [t[k] for t in trs for k in ("period", "offset", "end_exemptions")] + [len(bnd)]
    for col, step, value, coeff in bnd:
        args += [col, step, value] + list(coeff)
    out = subprocess.run([str(exe)] + [str(v) for v in args], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = {}
    for ln in out.stdout.splitlines():
        lines.setdefault(ln[0], []).append([int(x) for x in ln[1:].split()])
    keys = []
    for t in trs:
        key = (t["period"], t["offset"], t["end_exemptions"])
        if key not in keys:
            keys.append(key)
    assert lines["C"] == [[keys.index((t["period"], t["offset"], t["end_exemptions"])) for t in trs]] and len(keys) == 5
    assert lines["K"] == [list(dom.trace_points[o]) + [M.log2(dom.n // p) - 1, 2 * dom.blowup * p] for p, o, _ in keys]
    assert lines["E"] == [list(pt) for p, o, e in keys for pt in M.exemption_points(dom, dict(period=p, offset=o, end_exemptions=e))]
    order = sorted(range(len(bnd)), key=lambda k: bnd[k][1])             # stable
    assert lines["O"] == [order]
    steps, first = [], 0
    for step in sorted({b[1] for b in bnd}):
        members = [k for k in order if bnd[k][1] == step]
        const = R.ZERO
        for k in members:
            const = R.add(const, R.mul_base(R.elem(bnd[k][3]), CR.reduce_word(bnd[k][2])))
        steps.append([step] + list(dom.trace_points[step]) + [first, len(members)] + list(const))
        first += len(members)
    assert lines["S"] == steps
    lg = log2_trace + log2_blowup
    hbits = (lg + 1) // 2
    assert lines["T"] == [[hbits, 1 << hbits, 1 << (lg - hbits)] + list(CR.subgroup_generator(lg + 1)) + list(CR.subgroup_generator(lg))]
    # the table's rule gives every point of the coset
    gN, g2N = CR.subgroup_generator(lg), CR.subgroup_generator(lg + 1)
    for i in range(dom.N):
        lo, hi = CR.pmul(i & ((1 << hbits) - 1), gN), CR.padd(g2N, CR.pmul((i >> hbits) << hbits, gN))
        assert CR.padd(hi, lo) == dom.lde_points[i]
