"""The primitives of csrc/field.cuh, one call per row through lw_hip_field_pointwise_device, against plain Python integers
(tests/field_ops_ref.py) at operands the transforms never produce.

Every NTT, hash and prover test starts from pseudo-random elements and compares a whole transform; the final subtraction
of a Stark252 product is taken by under 1 % of such pairs, and fe_reduce_full's conditional + p by almost none.  Here
every operand is chosen - p - 1, zero and all-ones limbs, products that land exactly on p, the 93 inputs at which the
quotient estimate of fe_reduce_full is one too large, the sums of the BabyBear butterfly next to bb_reduce's
precondition - and the returned limbs are compared bit for bit; every output documented as canonical must be below p.
Every operand is inside the domain csrc/field_pointwise_ops.cuh documents: nothing here is meant to go wrong on the device.
tests/test_field_pointwise_cpu.py proves the reference and the coverage of the sets without a GPU."""
import numpy as np
import pytest

from tests import field_ops_ref as FR

pytestmark = pytest.mark.gpu
FILL = 0x5a5a5a5a5a5a5a5a
FIELD_IDS = [f.name for f in FR.FIELDS]
FIELD_OP_CASES = [(f.name, op) for f in FR.FIELDS for op in FR.FIELD_OPS if f.has(op) and op != FR.OP_MUL_LAZY_UNIFORM]


def to_device(a):
    """numpy (uint64 or uint32) -> a cuda tensor with the same bytes"""
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int64 if a.dtype == np.uint64 else np.int32)).cuda()


def from_device(t, dtype):
    return t.cpu().numpy().view(dtype)


def device_op(pw, op, a, b, n, out_shape, out_dtype, guard_rows=1, alias=None, stream=None):
    """The seam on packed arrays -> the n result rows.  guard_rows rows behind n are pre-filled and must come back
    untouched; alias 'a' / 'b': d_out is that operand's buffer (which then carries the guard rows)."""
    import torch
    from lambda_elliptic_curves_amd import field_ops
    fill = np.frombuffer(np.uint64(FILL).tobytes(), out_dtype)[0]
    guard = np.full((guard_rows,) + tuple(out_shape[1:]), fill, out_dtype)
    t_a = to_device(np.concatenate([a, guard]) if alias == "a" else a)
    t_b = None if b is None else to_device(np.concatenate([b, guard]) if alias == "b" else b)
    if alias:
        out = t_a if alias == "a" else t_b
    else:
        out = to_device(np.full((n + guard_rows,) + tuple(out_shape[1:]), fill, out_dtype))
    field_ops.field_pointwise_device(pw, op, t_a, t_b, n, out, stream=stream)
    torch.cuda.synchronize()
    got = from_device(out, out_dtype)
    assert got.shape[0] == n + guard_rows and (got[n:] == fill).all(), "rows past n were written"
    return got[:n]


def field_op(f, op, a_rows, b_rows, **kw):
    """rows of integers -> result integers"""
    n = len(b_rows) if op == FR.OP_MUL_LAZY_UNIFORM else len(a_rows)
    got = device_op(f.pw, op, FR.pack_rows(f, a_rows), FR.pack_rows(f, b_rows) if b_rows is not None else None, n,
                    (n, f.words), np.uint64, **kw)
    return FR.unpack(f, got)


def check_rows(f, op, a_rows, b_rows, want, **kw):
    """device == reference, bit for bit, and every canonical output below p"""
    got = field_op(f, op, a_rows, b_rows, **kw)
    if op in FR.CANONICAL:
        assert all(v < f.p for v in got), f"{f.name} {FR.OP_NAMES[op]}: an output is not a canonical residue"
    if got != want:
        i = next(i for i in range(len(want)) if got[i] != want[i])
        a = a_rows[0] if op == FR.OP_MUL_LAZY_UNIFORM else a_rows[i]
        show = lambda v: None if v is None else (tuple(hex(x) for x in v) if isinstance(v, tuple) else hex(v))
        raise AssertionError(f"{f.name} op {FR.OP_NAMES[op]} row {i} of {len(want)}: a = {show(a)}, "
                             f"b = {show(b_rows[i]) if b_rows else None}, got {hex(got[i])}, want {hex(want[i])}")
    return got


@pytest.mark.parametrize("name,op", FIELD_OP_CASES, ids=[f"{n}-{FR.OP_NAMES[op]}" for n, op in FIELD_OP_CASES])
def test_primitives_bit_exact_at_chosen_operands(name, op):
    f = FR.BY_NAME[name]
    a_rows, b_rows = FR.operands(name, op)
    assert FR.N_RANDOM < len(a_rows) < 3 * FR.N_RANDOM
    check_rows(f, op, a_rows, b_rows, FR.expected(name, op))


@pytest.mark.parametrize("name", FIELD_IDS)
def test_uniform_operand_product_gives_the_bytes_of_the_lazy_product(name):
    """Every member of E in turn as the single row of d_a, against every b of E': the reference's product, and byte for
    byte what MUL_LAZY returns for the same pairs (one launch over E x E')."""
    f = FR.BY_NAME[name]
    ed, wd = FR.edge_set(name), FR.wide_set(name)
    a_rows, b_rows = FR.operands(name, FR.OP_MUL_LAZY)
    npairs = len(ed) * len(wd)
    assert a_rows[:npairs] == [a for a in ed for _ in wd] and b_rows[:npairs] == wd * len(ed)
    want = FR.expected(name, FR.OP_MUL_LAZY)[:npairs]
    lazy = check_rows(f, FR.OP_MUL_LAZY, a_rows[:npairs], b_rows[:npairs], want)
    for j, a in enumerate(ed):
        got = check_rows(f, FR.OP_MUL_LAZY_UNIFORM, [a], wd, want[j * len(wd):(j + 1) * len(wd)])
        assert got == lazy[j * len(wd):(j + 1) * len(wd)]


def bb_device(op, a, b, **kw):
    n = len(a)
    got = device_op(FR.PW_FIELD_BABYBEAR, op, np.array(a, FR.BB_IN_DTYPE[op]), np.array(b, np.uint32) if b is not None else None, n,
                    (n,), FR.BB_OUT_DTYPE[op], **kw)
    return [int(v) for v in got]


@pytest.mark.parametrize("op", FR.BB_OPS, ids=[FR.OP_NAMES[op] for op in FR.BB_OPS])
def test_babybear_words_bit_exact(op):
    a, b = FR.bb_operands(op)
    want = FR.bb_expected(op)
    got = bb_device(op, a, b)
    assert all(v < FR.BB_P for v in got), "an output is not a canonical residue"
    bad = [i for i in range(len(want)) if got[i] != want[i]][:1]
    assert not bad, (f"babybear op {FR.OP_NAMES[op]} row {bad[0]} of {len(want)}: a = {a[bad[0]]:#x}, "
                     f"b = {b[bad[0]] if b else None}, got {got[bad[0]]:#x}, want {want[bad[0]]:#x}")


# ---------------------------------------------------------------- launch shapes, aliasing, streams
SHAPES = [1, 63, 64, 65, 4096 + 5]


def shape_rows(name, op, n):
    """n rows of the op's set: the last n, cycled, so that targeted rows are in for the longest launch"""
    a_rows, b_rows = FR.operands(name, op)
    idx = [(len(a_rows) - 1 - i) % len(a_rows) for i in range(n)]
    want = FR.expected(name, op)
    return [a_rows[i] for i in idx], ([b_rows[i] for i in idx] if b_rows else None), [want[i] for i in idx]


@pytest.mark.parametrize("n", SHAPES)
@pytest.mark.parametrize("name", FIELD_IDS)
def test_launch_shapes_leave_the_rows_behind_n_alone(name, n):
    f = FR.BY_NAME[name]
    for op in (FR.OP_MUL, FR.OP_DOT2, FR.OP_NEG):       # two operands, wide rows, one operand
        a, b, want = shape_rows(name, op, n)
        check_rows(f, op, a, b, want, guard_rows=3)


@pytest.mark.parametrize("n", SHAPES)
def test_babybear_launch_shapes(n):
    for op in (FR.OP_MUL, FR.OP_REDUCE64, FR.OP_TO_R64):
        a, b = FR.bb_operands(op)
        want = FR.bb_expected(op)
        idx = [(len(a) - 1 - i) % len(a) for i in range(n)]
        assert bb_device(op, [a[i] for i in idx], [b[i] for i in idx] if b else None, guard_rows=3) == [want[i] for i in idx]


@pytest.mark.parametrize("alias", ["a", "b"])
@pytest.mark.parametrize("name", FIELD_IDS)
def test_output_may_be_an_operand(name, alias):
    f = FR.BY_NAME[name]
    for op in (FR.OP_MUL, FR.OP_SUB, FR.OP_ADD2P_SUB_RAW) + ((FR.OP_SQR, FR.OP_REDUCE_FULL) if alias == "a" else (FR.OP_MUL_LAZY_UNIFORM,)):
        if op == FR.OP_MUL_LAZY_UNIFORM:                # d_out may be d_b; d_a is the single row
            a, b = [FR.edge_set(name)[3]], FR.wide_set(name) * 4
            want = [FR.op_mul_lazy(f, a[0], x) for x in b]
        else:
            a, b, want = shape_rows(name, op, 4096 + 5)
        check_rows(f, op, a, b, want, guard_rows=2, alias=alias)


@pytest.mark.parametrize("alias", ["a", "b"])
def test_babybear_output_may_be_an_operand(alias):
    for op in (FR.OP_MUL, FR.OP_ADD, FR.OP_SUB):
        a, b = FR.bb_operands(op)
        assert bb_device(op, a, b, guard_rows=2, alias=alias) == FR.bb_expected(op)


def test_on_a_stream_of_the_callers():
    import torch
    f = FR.STARK252
    a, b, want = shape_rows(f.name, FR.OP_MUL_LAZY, 4096 + 5)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        check_rows(f, FR.OP_MUL_LAZY, a, b, want, stream=s.cuda_stream)
