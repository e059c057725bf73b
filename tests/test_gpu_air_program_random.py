"""Random AIR programs (tests/air_program_gen.py: DAGs through stark.compile_transitions, and raw op lists) on every device
interpreter of lw_stark_air_op_t, bit for bit against the Python models: csrc/stark_air.hip over Stark252 and Fr381
(air_program_ref.run_all), the fused passes of csrc/ext_round2.cuh over Goldilocks/Fp2 and BabyBear/Fp4 (ext_round2_ref.evaluate),
their RAP form with typed temporaries in LDS (ext_rap_ref.evaluate) and csrc/circle_round2.cuh over Mersenne31/QM31
(circle_round2_ref.evaluate).  tests/test_air_program_gen_cpu.py proves the same lists on the host.

Shapes: trace 2^3, blow-up 4 (N = 32: under one block of 256, every row offset wraps) for 12 seeds a backend, and trace 2^8,
blow-up 4 (N = 1024: four blocks, the wrap crosses a block) for 2 seeds a backend with programs of at most 200 ops.
LW_AIR_RANDOM_EXTRA_SEEDS=K adds K seeds at the small shape.  The device and model calls are those of the modules that test
each backend by hand."""
import numpy as np
import pytest

from lambda_elliptic_curves_amd import stark
from tests import air_program_gen as G
from tests import air_program_ref as A
from tests import circle_round2_ref as CM
from tests import ext_rap_ref as R
from tests import ext_round2_ref as M
from tests import stark_round2_ref as R2
from tests import test_gpu_air_program as T_AIR
from tests import test_gpu_circle_round2 as T_M31
from tests import test_gpu_ext_rap as T_RAP
from tests import test_gpu_ext_round2 as T_EXT

pytestmark = pytest.mark.gpu
SHAPES = {"small": G.SMALL, "large": G.LARGE}


def cases(typed):
    """(size, seed) of every program of the lists that compiled or was drawn raw"""
    return [(size, e[0]) for (t, size), entries in G.program_lists(stark).items() if t == typed for e in entries if e[1] != "refused"]


def program(typed, size, seed):
    _seed, _kind, ops, T, _exprs = next(e for e in G.program_lists(stark)[(typed, size)] if e[0] == seed)
    return ops, T, stark.AirProgram(np.array(ops, dtype=stark.AIR_OP_DTYPE), T)


def mixed(rng, p, n, draw=None):
    """n canonical values: three in four random, the rest from {0, 1, p - 1}"""
    draw = draw or (lambda: int.from_bytes(rng.bytes(40), "big") % p)
    edge = [0, 1, p - 1]
    return [edge[int(rng.integers(0, 3))] if rng.random() < 0.25 else draw() for _ in range(n)]


def nonzero_elems(rng, p, width, n):
    out = [tuple(int.from_bytes(rng.bytes(16), "big") % (p - 1) + 1 for _ in range(width)) for _ in range(n)]
    assert all(all(c) for c in out)
    return out


def transitions_of(T, seed, coeffs):
    trs = [dict(t, coeff=coeffs[c]) for c, t in enumerate(G.descriptors_of(T, seed))]
    assert T < 2 or 2 <= len({(t["period"], t["offset"], t["end_exemptions"]) for t in trs}) <= 3
    return trs


IDS = lambda cs: [f"{size}-{seed}" for size, seed in cs]


# ---- csrc/stark_air.hip
@pytest.mark.parametrize("size,seed", cases(False), ids=IDS(cases(False)))
@pytest.mark.parametrize("field", T_AIR.FIELDS)
def test_transition_rows(field, size, seed):
    p = T_AIR.MODULI[field]
    ops, T, prog = program(False, size, seed)
    log2_trace, log2_blowup = SHAPES[size]
    dom = R2.Domain(p, log2_trace, log2_blowup, 3)
    rng = np.random.default_rng(seed + 7000)
    cols = [mixed(rng, p, dom.N) for _ in range(G.N_COLS)]
    consts = mixed(rng, p, G.N_CONSTS)
    want = A.run_all(ops, dom, cols, consts, T)
    T_AIR.assert_rows(field, T_AIR.run_device(field, prog, dom, cols, consts, log2_trace, log2_blowup), want, dom.N)


# ---- the fused passes of csrc/ext_round2.cuh
@pytest.mark.parametrize("size,seed", cases(False), ids=IDS(cases(False)))
@pytest.mark.parametrize("field", T_EXT.FIELDS)
def test_fused_pass(field, size, seed):
    F = M.FIELDS[field]
    ops, T, prog = program(False, size, seed)
    dom = M.domain(F, SHAPES[size][0], SHAPES[size][1], 3)
    rng = np.random.default_rng(seed + 7100)
    cols = [mixed(rng, F.p, dom.N) for _ in range(G.N_COLS)]
    consts = mixed(rng, F.p, G.N_CONSTS)
    coeffs = nonzero_elems(rng, F.p, F.width, T + 3)
    boundary = [(0, 0, F.p - 1, coeffs[T]), (2, dom.n - 1, 7, coeffs[T + 1]), (1, 0, 0, coeffs[T + 2])]
    T_EXT.check(F, dom, cols, prog, consts, boundary, transitions_of(T, seed, coeffs))


# ---- their RAP form: 2 auxiliary columns, 2 constants of the extension
@pytest.mark.parametrize("size,seed", cases(True), ids=IDS(cases(True)))
@pytest.mark.parametrize("field", T_RAP.FIELDS)
def test_fused_rap_pass(field, size, seed):
    F = M.FIELDS[field]
    ops, T, prog = program(True, size, seed)
    assert (G.N_XCOLS, G.N_XCONSTS) == (2, 2)
    dom = M.domain(F, SHAPES[size][0], SHAPES[size][1], 3)
    rng = np.random.default_rng(seed + 7200)
    cols = [mixed(rng, F.p, dom.N) for _ in range(G.N_COLS)]
    aux = [list(zip(*[mixed(rng, F.p, dom.N) for _ in range(F.width)])) for _ in range(G.N_XCOLS)]
    consts = mixed(rng, F.p, G.N_CONSTS)
    xconsts = [tuple(mixed(rng, F.p, F.width)) for _ in range(G.N_XCONSTS)]
    coeffs = nonzero_elems(rng, F.p, F.width, T + 4)
    boundary = [(0, 0, F.p - 1, coeffs[T], False), (1, dom.n - 1, coeffs[T + 3], coeffs[T + 1], True), (0, 1, M.lift(F, 5), coeffs[T + 2], True)]
    T_RAP.check_rap(F, dom, cols, aux, prog, consts, xconsts, boundary, transitions_of(T, seed, coeffs))


# ---- csrc/circle_round2.cuh
@pytest.mark.parametrize("size,seed", cases(False), ids=IDS(cases(False)))
def test_circle_fused_pass(size, seed):
    P = CM.P
    ops, T, prog = program(False, size, seed)
    dom = CM.Domain(*SHAPES[size])
    rng = np.random.default_rng(seed + 7300)
    word = lambda: int(rng.integers(0, P))
    cols = [mixed(rng, P, dom.N, word) for _ in range(G.N_COLS)]
    consts = mixed(rng, P, G.N_CONSTS, word)
    coeffs = nonzero_elems(rng, P, 4, T + 2)
    boundary = [(0, 0, P - 1, coeffs[T]), (2, dom.n - 1, 7, coeffs[T + 1])]
    T_M31.check(dom, cols, prog, consts, boundary, transitions_of(T, seed, coeffs))
