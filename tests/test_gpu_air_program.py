"""AIR transition programs on the device (csrc/stark_air.hip) against tests/air_program_ref.py, the interpreter of the op
list in Python integers, and against the Stone-compatibility case of tests/golden/stark_round2.json.  Field arithmetic is
exact: every comparison is byte equality in the stored (Montgomery) form."""
import functools
import json
import os

import numpy as np
import pytest

from oracle import bigint_def as D
from tests import air_program_ref as A
from tests import stark_round2_ref as R2

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODULI = {"stark252": D.P_STARK252, "fr381": D.P_FR381}
FIELDS = ["stark252", "fr381"]


def S():
    from lambda_elliptic_curves_amd import stark
    return stark


def fld(name):
    from lambda_elliptic_curves_amd import fft
    return {"stark252": fft.Stark252PrimeField, "fr381": fft.FrField}[name]


def cuda(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).cuda()


def host(t):
    return t.cpu().numpy().view(np.uint64)


def program_of(ops, n_transitions):
    return S().AirProgram(np.array(ops, dtype=S().AIR_OP_DTYPE), n_transitions)


def run_device(name, program, dom, cols, consts, log2_trace, log2_blowup, lens=None, t_out=None):
    p = MODULI[name]
    t_cols = [cuda(R2.to_stored(p, c)) for c in cols]
    return S().transition_evaluations_device(fld(name), program, R2.to_stored(p, consts) if consts else None, t_cols, log2_trace,
                                             log2_blowup, col_log2_len=lens, t_out=t_out)


def assert_rows(name, t_out, want, N):
    p = MODULI[name]
    got = host(t_out)
    assert got.shape[0] == len(want)
    for c, row in enumerate(want):
        assert np.array_equal(got[c, :N], R2.to_stored(p, row)), (name, c)


@functools.lru_cache(maxsize=None)
def example(name, field, log2_trace, log2_blowup):
    """(program, dom, cols, lens, consts, the reference's T rows), computed once per case"""
    p = MODULI[field]
    program = S().compile_transitions(A.AIRS[name][0](S()))
    dom, cols, lens, consts = A.air_case(name, p, log2_trace, log2_blowup, 1000 + log2_trace)
    return program, dom, cols, lens, consts, A.run_all(program.ops, dom, cols, consts, program.n_transitions)


# ---- 1. the Stone-compatibility case

def test_stone_case_rows_and_composition_root():
    with open(os.path.join(ROOT, "tests", "golden", "stark_round2.json")) as f:
        golden = json.load(f)
    p, F = D.P_STARK252, fld("stark252")
    dom, lde, boundary, transitions, (t0, t1) = R2.fibonacci_2_cols_shifted_case(golden)
    st = S()
    program = st.compile_transitions([st.cell(0, 1) - st.cell(1), st.cell(1, 1) - st.cell(0) - st.cell(1)])
    t_cols = [cuda(R2.to_stored(p, c)) for c in lde]
    t_rows = st.transition_evaluations_device(F, program, None, t_cols, golden["log2_trace"], golden["log2_blowup"])
    assert_rows("stark252", t_rows, [t0, t1], dom.N)
    b, t = R2.stored_tables(p, boundary, transitions)
    _parts, _lens, _lde, _nodes, root = st.round2_program_device(F, t_cols, golden["log2_trace"], golden["log2_blowup"],
                                                                 R2.stored_one(p, golden["coset_offset"]), b, t, program, None, golden["n_parts"])
    assert root.hex() == golden["composition_root"]


# ---- 2. the reference's example AIRs, N = 32: under one block, the last row * blowup rows wrap

@pytest.mark.parametrize("field", FIELDS)
@pytest.mark.parametrize("name", ["simple_fib", "quadratic", "rom", "fib_rap", "periodic"])
def test_example_airs_match_the_interpreter(name, field):
    program, dom, cols, lens, consts, want = example(name, field, 3, 2)
    assert dom.N == 32 and (lens is None) == (name != "periodic")
    if name == "periodic":
        assert lens == [5, 3] and len(cols[1]) == 8
    assert_rows(field, run_device(field, program, dom, cols, consts, 3, 2, lens), want, dom.N)


# ---- 3. several blocks: N = 1024, the wrap crosses a block boundary

@pytest.mark.parametrize("field", FIELDS)
@pytest.mark.parametrize("name", ["rom", "periodic"])
def test_example_airs_over_several_blocks(name, field):
    program, dom, cols, lens, consts, want = example(name, field, 8, 2)
    assert dom.N == 1024
    assert_rows(field, run_device(field, program, dom, cols, consts, 8, 2, lens), want, dom.N)


# ---- 4. edge operands

def edge_program():
    """Row i of N = 16 holds the pair (a, b) = (edge[i // 4], edge[i % 4]) in columns 0 and 1; the constants are the edge
    values.  a op b for every op and every kind of operand (cell, constant, temporary), -a, and a * (p - 1)^64."""
    ops, T = [], 0

    def emit():
        nonlocal T
        ops.append((A.EMIT, 0, T, 0))
        T += 1
    for op in (A.ADD, A.SUB, A.MUL):
        ops.extend([(A.LOAD, A.CELL, 0, 0), (op, A.CELL, 1, 0)])
        emit()
    ops.extend([(A.LOAD, A.CELL, 0, 0), (A.NEG, 0, 0, 0)])
    emit()
    ops.append((A.LOAD, A.CELL, 0, 0))
    ops.extend([(A.MUL, A.CONST, 2, 0)] * 64)                  # constant 2 is p - 1
    emit()
    for k in range(4):
        for op in (A.ADD, A.SUB, A.MUL):
            ops.extend([(A.LOAD, A.CELL, 0, 0), (op, A.CONST, k, 0)])
            emit()
    ops.extend([(A.LOAD, A.CELL, 1, 0), (A.STORE, 0, 3, 0)])
    for op in (A.ADD, A.SUB, A.MUL):
        ops.extend([(A.LOAD, A.CELL, 0, 0), (op, A.TMP, 3, 0)])
        emit()
    ops.extend([(A.LOAD, A.CELL, 1, 0), (A.NEG, 0, 0, 0), (A.NEG, 0, 0, 0), (A.STORE, 0, 0, 0), (A.LOAD, A.CONST, 0, 0), (A.SUB, A.TMP, 0, 0)])
    emit()                                                      # 0 - (-(-b))
    return ops, T


@pytest.mark.parametrize("field", FIELDS)
def test_edge_operands(field):
    p = MODULI[field]
    edge = A.edge_values(p)
    assert edge[:3] == [0, 1, p - 1] and 1 < edge[3] < p - 1
    dom = R2.Domain(p, 3, 1, 3)
    cols = [[edge[i // 4] for i in range(16)], [edge[i % 4] for i in range(16)]]
    pairs = set(zip(*cols))
    assert (p - 1, p - 1) in pairs and (0, p - 1) in pairs and (0, 0) in pairs      # (p-1) op (p-1), 0 - (p-1), -0
    ops, T = edge_program()
    assert sum(1 for k in range(len(ops) - 63) if all(o == (A.MUL, A.CONST, 2, 0) for o in ops[k:k + 64])) == 1
    want = A.run_all(ops, dom, cols, edge, T)
    assert want[1][cols[0].index(0) + 2] == 1 and want[3][0] == 0 and want[4][8] == p - 1      # 0 - (p-1), -0, (p-1)^65
    t_out = run_device(field, program_of(ops, T), dom, cols, edge, 3, 1)
    assert all(v < p for v in R2.O.array_to_ints(host(t_out).reshape(-1, 4)))
    assert_rows(field, t_out, want, dom.N)


# ---- 5. limits

def limits_program(n):
    """4096 ops, the 8 temporaries alive at once, 256 constants, row = n - 1, constraints emitted as 3, 2, 1, 0, 4"""
    ops = [(A.LOAD, A.CELL, 0, n - 1)]
    for t in range(A.MAX_TMPS):
        ops.extend([(A.ADD, A.CONST, t, 0), (A.STORE, 0, t, 0)])
    for c in reversed(range(4)):
        ops.extend([(A.MUL, A.TMP, 2 * c, 0), (A.ADD, A.TMP, 2 * c + 1, 0), (A.EMIT, 0, c, 0)])
    k = 0
    while len(ops) < A.MAX_OPS - 1:
        ops.append((A.MUL if k % 3 == 2 else A.ADD, A.CONST if k % 5 else A.CELL, k % A.MAX_CONSTS if k % 5 else 0, 0 if k % 5 else k % n))
        k += 1
    ops.append((A.EMIT, 0, 4, 0))
    return ops, 5


@pytest.mark.parametrize("field", FIELDS)
def test_a_program_at_every_limit(field):
    p = MODULI[field]
    dom = R2.Domain(p, 4, 2, 3)
    ops, T = limits_program(dom.n)
    assert len(ops) == A.MAX_OPS and dom.N == 64
    assert {o[2] for o in ops if o[0] <= A.MUL and o[1] == A.CONST} == set(range(A.MAX_CONSTS))
    assert max(o[3] for o in ops) == dom.n - 1
    cols = [A.fill(p, dom.N, 21)]
    consts = A.fill(p, A.MAX_CONSTS, 22)
    want = A.run_all(ops, dom, cols, consts, T)
    program = program_of(ops, T)
    assert program.n_tmps == A.MAX_TMPS and program.n_consts == A.MAX_CONSTS
    assert_rows(field, run_device(field, program, dom, cols, consts, 4, 2), want, dom.N)


# ---- 6. output layout

def test_a_stride_above_N_leaves_the_gap_alone_and_a_short_output_is_refused():
    import torch
    from lambda_elliptic_curves_amd import errors
    program, dom, cols, lens, consts, want = example("rom", "stark252", 3, 2)
    N, T, gap = dom.N, program.n_transitions, 8
    sentinel = 0x5a5a5a5a5a5a5a5a
    t_out = torch.full((T, N + gap, 4), sentinel, dtype=torch.int64, device="cuda")
    got = run_device("stark252", program, dom, cols, consts, 3, 2, lens, t_out=t_out)
    assert got.data_ptr() == t_out.data_ptr()
    assert_rows("stark252", t_out, want, N)
    assert (host(t_out)[:, N:] == np.uint64(sentinel)).all()
    short = torch.zeros((T * N - 1) * 4, dtype=torch.int64, device="cuda")
    with pytest.raises(errors.LengthMismatch):
        run_device("stark252", program, dom, cols, consts, 3, 2, lens, t_out=short)
    with pytest.raises(errors.LengthMismatch):     # the last row does not fit its stride
        run_device("stark252", program, dom, cols, consts, 3, 2, lens, t_out=torch.zeros((T, N - 1, 4), dtype=torch.int64, device="cuda"))
    assert not host(short).any()


# ---- 7. the host-array twin

@pytest.mark.parametrize("field", FIELDS)
@pytest.mark.parametrize("name", ["rom", "periodic"])
def test_host_twin_equals_the_device_form(name, field):
    p = MODULI[field]
    program, dom, cols, lens, consts, want = example(name, field, 3, 2)
    got = S().transition_evaluations(fld(field), program, R2.to_stored(p, consts) if consts else None, [R2.to_stored(p, c) for c in cols],
                                     3, 2, col_log2_len=lens)
    assert got.shape == (program.n_transitions, dom.N, 4)
    assert np.array_equal(got, host(run_device(field, program, dom, cols, consts, 3, 2, lens)))
    assert np.array_equal(got, np.stack([R2.to_stored(p, row) for row in want]))
