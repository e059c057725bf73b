"""The field-arithmetic seam without a GPU: the argument checks of lw_hip_field_pointwise_device, which all return before
any device work; the reference of tests/test_gpu_field_pointwise.py (tests/field_ops_ref.py) against independent code:
the op table itself compiled for the host under AddressSanitizer and UBSan, the oracle, and the model of the emitted
Stark252 columns; and the coverage conditions of the operand sets, on the reference alone."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

from oracle import oracle as O
from tests import ec_formulas_ref as E
from tests import field_ops_ref as FR
from tests import test_mac_chain_bounds_cpu as M
from tools import gen_mac_chains as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELD_IDS = [f.name for f in FR.FIELDS]


@pytest.fixture(scope="module")
def lib():
    from lambda_elliptic_curves_amd import _lib
    return _lib, _lib.lib()


def test_enums_match_the_binding(lib):
    L, _ = lib
    assert [getattr(L, "FIELD_OP_" + n.upper()) for n in FR.OP_NAMES] == list(range(22))
    assert [f.pw for f in FR.FIELDS] == [L.PW_FIELD_STARK252, L.PW_FIELD_FR381, L.PW_FIELD_FR254, L.PW_FIELD_FP381, L.PW_FIELD_FP254]
    assert FR.PW_FIELD_BABYBEAR == L.PW_FIELD_BABYBEAR


def test_pointwise_argument_checks(lib):
    L, dll = lib
    buf = np.zeros((64, 6), np.uint64)
    base = buf.ctypes.data + (-buf.ctypes.data) % 16
    p, q, r = (C.c_void_p(base + 1024 * k) for k in range(3))
    odd = C.c_void_p(base + 8)
    call = dll.lw_hip_field_pointwise_device
    BAD = L.ERR_BAD_ARG
    for f in FR.FIELDS:
        for op in range(22):
            two = op in FR.TWO_OPERANDS
            b = q if two else None
            if not f.has(op):                                                   # DOT4 on Fr381, the BabyBear ops
                assert op > FR.OP_INV or (f is FR.FR381 and op == FR.OP_DOT4)
                assert call(f.pw, op, p, b, 4, r, None) == BAD and b"has no op" in dll.lw_hip_last_error()
                assert call(f.pw, op, None, None, 0, None, None) == BAD         # ... even with n = 0
                continue
            assert call(f.pw, op, None, None, 0, None, None) == L.OK            # n = 0: nothing touched, no device
            assert call(f.pw, op, None, b, 4, r, None) == BAD                   # null a
            assert call(f.pw, op, p, b, 4, None, None) == BAD                   # null out
            assert call(f.pw, op, p, None if two else q, 4, r, None) == BAD     # b missing / superfluous
            assert call(f.pw, op, odd, b, 2, r, None) == BAD                    # misaligned
            assert call(f.pw, op, p, b, 2, odd, None) == BAD
            assert call(f.pw, op, p, b, 4, C.c_void_p(base + 16), None) == BAD  # out inside a, not row for row
            if two:
                assert call(f.pw, op, p, b, 4, C.c_void_p(base + 1024 + 16), None) == BAD
            if op in (FR.OP_DOT2, FR.OP_DOT4, FR.OP_MUL_LAZY_UNIFORM):          # out == a where the rows differ in length
                assert call(f.pw, op, p, b, 4, p, None) == BAD and b"overlaps" in dll.lw_hip_last_error()
            if op in (FR.OP_DOT2, FR.OP_DOT4):
                assert call(f.pw, op, p, b, 4, q, None) == BAD
    bb = L.PW_FIELD_BABYBEAR
    for op in range(22):
        if op not in FR.BB_OPS:
            assert call(bb, op, p, q if op in FR.TWO_OPERANDS else None, 4, r, None) == BAD
            continue
        two = op in FR.TWO_OPERANDS
        b = q if two else None
        assert call(bb, op, None, None, 0, None, None) == L.OK
        assert call(bb, op, None, b, 4, r, None) == BAD
        assert call(bb, op, p, b, 4, None, None) == BAD
        assert call(bb, op, p, None if two else q, 4, r, None) == BAD
        assert call(bb, op, odd, b, 4, r, None) == BAD
        if FR.BB_IN_DTYPE[op] != FR.BB_OUT_DTYPE[op]:                           # out == a across word sizes
            assert call(bb, op, p, b, 4, p, None) == BAD
    for field in (6, -1):
        assert call(field, FR.OP_NEG, p, None, 4, r, None) == BAD               # bad field
        assert call(field, FR.OP_NEG, None, None, 0, None, None) == BAD
    for op in (22, -1):
        assert call(0, op, p, q, 4, r, None) == BAD                             # bad op
        assert call(0, op, None, None, 0, None, None) == BAD


@pytest.mark.parametrize("name", FIELD_IDS)
def test_moduli_are_the_oracle_moduli(name):
    f = FR.BY_NAME[name]
    prm = O.field_params(f.oracle)
    assert prm["q"] == f.p and prm["one"] == f.R % f.p and prm["r2"] == f.R * f.R % f.p


# ---------------------------------------------------------------- the op table on the host, under the sanitizers
def _job(field, op, n, a, b):
    return struct.pack("<IIQ", field, op, n) + a.tobytes() + (b.tobytes() if b is not None else b"")


@pytest.fixture(scope="module")
def host_results(tmp_path_factory):
    """every vector of every field and op through tests/field_pointwise_host_main.cpp, one child process:
    -> {(field name or 'babybear', op, uniform a or None): result array}"""
    tmp = tmp_path_factory.mktemp("field_pointwise_host")
    exe, fin, fout = tmp / "field_pointwise_host", tmp / "in.bin", tmp / "out.bin"
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-Wno-shift-count-overflow", "-o", str(exe), os.path.join(ROOT, "tests", "field_pointwise_host_main.cpp")])
    jobs, blob = [], []
    for f in FR.FIELDS:
        for op in FR.FIELD_OPS:
            if not f.has(op):
                continue
            if op == FR.OP_MUL_LAZY_UNIFORM:
                wd = FR.wide_set(f.name)
                for a in FR.edge_set(f.name):
                    jobs.append((f.name, op, a, len(wd), 8 * f.words))
                    blob.append(_job(f.pw, op, len(wd), FR.pack(f, [a]), FR.pack(f, wd)))
                continue
            a_rows, b_rows = FR.operands(f.name, op)
            jobs.append((f.name, op, None, len(a_rows), 8 * f.words))
            blob.append(_job(f.pw, op, len(a_rows), FR.pack_rows(f, a_rows), FR.pack_rows(f, b_rows) if b_rows else None))
    for op in FR.BB_OPS:
        a, b = FR.bb_operands(op)
        jobs.append(("babybear", op, None, len(a), np.dtype(FR.BB_OUT_DTYPE[op]).itemsize))
        blob.append(_job(FR.PW_FIELD_BABYBEAR, op, len(a), np.array(a, FR.BB_IN_DTYPE[op]), np.array(b, np.uint32) if b else None))
    fin.write_bytes(b"".join(blob))
    out = subprocess.run([str(exe), str(fin), str(fout)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and out.stdout.split() == ["ok", str(len(jobs))], (out.returncode, out.stdout, out.stderr[-3000:])
    raw = fout.read_bytes()
    assert len(raw) == sum(n * row for *_, n, row in jobs)
    res, off = {}, 0
    for name, op, uni, n, row in jobs:
        res[(name, op, uni)] = raw[off:off + n * row]
        off += n * row
    return res


def _first_mismatch(f, op, a_rows, b_rows, got, want):
    for i, (g, w) in enumerate(zip(got, want)):
        if g != w:
            return (f"{f.name} {FR.OP_NAMES[op]} row {i} of {len(want)}: a = {a_rows[i]:#x}" if not isinstance(a_rows[i], tuple) else
                    f"{f.name} {FR.OP_NAMES[op]} row {i} of {len(want)}: a = {a_rows[i]}") + f", b = {b_rows[i] if b_rows else None}, got {g:#x}, want {w:#x}"
    return None


@pytest.mark.parametrize("name", FIELD_IDS)
def test_host_build_of_the_op_table_equals_the_reference(name, host_results):
    f = FR.BY_NAME[name]
    ran = 0
    for op in FR.FIELD_OPS:
        if not f.has(op) or op == FR.OP_MUL_LAZY_UNIFORM:
            continue
        a_rows, b_rows = FR.operands(name, op)
        want = FR.expected(name, op)
        got = FR.unpack(f, np.frombuffer(host_results[(name, op, None)], np.uint64))
        assert len(got) == len(want) >= FR.N_RANDOM
        assert got == want, _first_mismatch(f, op, a_rows, b_rows, got, want)
        if op in FR.CANONICAL:
            assert all(v < f.p for v in want)
        elif op in (FR.OP_MUL_LAZY,):
            assert all(v < 2 * f.p for v in want)
        assert all(0 <= v < f.R for v in want)
        ran += 1
    assert ran == (17 if f is FR.FR381 else 18)
    wd = FR.wide_set(name)
    for a in FR.edge_set(name):                       # the uniform product: the bytes of MUL_LAZY on the same pairs
        got = FR.unpack(f, np.frombuffer(host_results[(name, FR.OP_MUL_LAZY_UNIFORM, a)], np.uint64))
        assert got == [FR.op_mul_lazy(f, a, b) for b in wd], (name, hex(a))


def test_host_build_of_the_babybear_ops_equals_the_reference(host_results):
    for op in FR.BB_OPS:
        a, b = FR.bb_operands(op)
        want = FR.bb_expected(op)
        got = [int(v) for v in np.frombuffer(host_results[("babybear", op, None)], FR.BB_OUT_DTYPE[op])]
        bad = [i for i in range(len(want)) if got[i] != want[i]][:1]
        assert not bad, f"babybear {FR.OP_NAMES[op]} row {bad[0]}: a = {a[bad[0]]}, b = {b[bad[0]] if b else None}, got {got[bad[0]]}, want {want[bad[0]]}"
        assert all(v < FR.BB_P for v in want)


@pytest.mark.parametrize("name", FIELD_IDS)
def test_reference_products_are_the_oracle_products(name):
    """MUL (rows with both operands canonical, which is what the oracle takes) and FROM_MONT against the oracle"""
    f = FR.BY_NAME[name]
    a_rows, b_rows = FR.operands(name, FR.OP_MUL)
    want = FR.expected(name, FR.OP_MUL)
    rows = [i for i in range(len(a_rows)) if a_rows[i] < f.p and b_rows[i] < f.p]
    assert len(rows) > 2000
    for i in rows:
        assert O.fe_op(f.oracle, O.OP_MUL, a_rows[i], b_rows[i]) == want[i], (name, i)
    a_rows, _ = FR.operands(name, FR.OP_FROM_MONT)
    want = FR.expected(name, FR.OP_FROM_MONT)
    for i, a in enumerate(a_rows):
        assert O.from_mont(f.oracle, a) == want[i], (name, i)


# ---------------------------------------------------------------- the Stark252 vectors through the model of the emitted columns
class Reach:
    """model_product with run_column watched: per column, the largest addend handed in and the largest value of the low
    pair after the column's last MAC that has no add-with-carry behind it"""

    def __init__(self, a_lt_p):
        self.a_lt_p = a_lt_p
        self.col = {id(prog): k for k, prog in enumerate(M.COLS[a_lt_p])}
        self.addend = [0] * (2 * M.N - 1)
        self.carryless = [0] * (2 * M.N - 1)

    def product(self, a, b):
        inner = M.run_column

        def watched(prog, init, al, bl, m):
            k = self.col[id(prog)]
            self.addend[k] = max(self.addend[k], init)
            val = lambda o: o[1] if o[0] == "imm" else {"a": al, "b": bl, "m": m, "p": M.P}[o[0]][o[1]]
            s = init
            for q, ins in enumerate(prog):
                if ins[0] != "mad" or (q + 1 < len(prog) and prog[q + 1][0] != "mad"):
                    break
                s += val(ins[1]) * val(ins[2])
                self.carryless[k] = max(self.carryless[k], s)
            return inner(prog, init, al, bl, m)

        M.run_column = watched
        try:
            return M.model_product(a, b, self.a_lt_p)
        finally:
            M.run_column = inner


def dropped_columns(a_lt_p):
    """columns (but the last, whose top word is not computed at all) with a MAC that has no add-with-carry behind it on
    the strength of a bound on the a*b operands or on the addend: column k -> the proven bound of the running sum"""
    out = {}
    for k in range(1, 2 * M.N - 2):                   # column 0 is one 32 x 32 MAC on a zero addend: nothing to drop
        plan = G.fused_col_plan(M.P, k, a_lt_p)
        ab = [q for q, mac in enumerate(plan["macs"]) if mac[0] == "ab" and not mac[3]]
        if ab:
            out[k] = dict(plan["proof"])[ab[-1]]
    return out


@pytest.fixture(scope="module")
def reach():
    """-> {a_lt_p: (targeted Reach, random Reach)} over the Stark252 MUL (general columns) and MUL_LAZY (a < p columns) rows,
    every product also compared with the reference"""
    f = FR.STARK252
    out = {}
    for a_lt_p, op in ((False, FR.OP_MUL), (True, FR.OP_MUL_LAZY)):
        a_rows, b_rows = FR.operands(f.name, op)
        want = FR.expected(f.name, op)
        nt = FR.n_targeted(f.name, op)
        tgt, rnd = Reach(a_lt_p), Reach(a_lt_p)
        for i, (a, b) in enumerate(zip(a_rows, b_rows)):
            t, lost = (tgt if i < nt else rnd).product(a, b)
            assert not lost, (hex(a), hex(b))
            assert t == FR.op_mul_lazy(f, a, b), (hex(a), hex(b))
            assert want[i] == (t if op == FR.OP_MUL_LAZY or t < f.p else t - f.p)
        out[a_lt_p] = (tgt, rnd)
    return out


def test_stark252_product_vectors_through_the_column_model(reach):
    assert set(reach) == {False, True}                # the comparisons are the fixture's


def reach_table(reach):
    lines = []
    for a_lt_p in (False, True):
        tgt, rnd = reach[a_lt_p]
        drop = dropped_columns(a_lt_p)
        lines.append(f"{'fe_mul_lazy: FusedCol<Stark252, K, true>, a < p' if a_lt_p else 'fe_mul: FusedCol<Stark252, K, false>, any operands'}")
        lines.append("  K  addend: proven bound        targeted rows         random rows | carry-less sum: bound    targeted (short by)            random")
        for k in range(2 * M.N - 1):
            plan = G.fused_col_plan(M.P, k, a_lt_p)
            line = f" {k:2d}  {plan['carry_in']:#20x} {tgt.addend[k]:#20x} {rnd.addend[k]:#20x} |"
            if k in drop:
                line += f" {drop[k]:#18x} {tgt.carryless[k]:#18x} ({drop[k] - tgt.carryless[k]:#x}) {rnd.carryless[k]:#18x}"
            lines.append(line.rstrip())
    return lines


def test_targeted_rows_reach_further_into_the_fused_columns_than_random_rows(reach):
    """Per column of the Stark252 product: the largest addend carried in over the vector set, the bound tools/gen_mac_chains.py
    proves, and the best of the 4096 random rows alone; and, where an a*b MAC has its add-with-carry dropped, the same
    three for the running sum the proof bounds.  profiles/field_operand_reach.txt holds the printed table."""
    lines = reach_table(reach)
    print("\n".join(lines))
    text = open(os.path.join(ROOT, "profiles", "field_operand_reach.txt")).read()
    for ln in lines:
        assert ln in text, "profiles/field_operand_reach.txt is stale: " + ln
    for a_lt_p in (False, True):
        tgt, rnd = reach[a_lt_p]
        drop = dropped_columns(a_lt_p)
        assert sorted(drop) == ([1, 2] if not a_lt_p else [1, 2] + list(range(7, 14)))
        for k in range(2 * M.N - 1):
            assert rnd.addend[k] <= tgt.addend[k] <= G.fused_col_plan(M.P, k, a_lt_p)["carry_in"]
        for k, bound in drop.items():
            assert tgt.carryless[k] <= bound < 1 << 64
            assert tgt.addend[k] > rnd.addend[k], (a_lt_p, k)
            assert tgt.carryless[k] > rnd.carryless[k], (a_lt_p, k)


# ---------------------------------------------------------------- coverage of the operand sets, on the reference alone
@pytest.mark.parametrize("name", FIELD_IDS)
def test_vector_sets_meet_their_coverage_conditions(name):
    f = FR.BY_NAME[name]
    p = f.p
    assert set(E.edge_values(p, f.words, 11)) < set(FR.edge_set(name)) and len(set(E.edge_values(p, f.words, 11))) >= 30
    for op in (FR.OP_MUL, FR.OP_SQR, FR.OP_MUL_LAZY):          # both sides of the final subtraction
        a_rows, b_rows = FR.operands(name, op)
        t = [FR.lazy(f, a * (b_rows[i] if b_rows else a)) for i, a in enumerate(a_rows)]
        assert all(v < 2 * p for v in t)
        assert sum(v >= p for v in t) >= FR.N_EACH_SIDE and sum(v < p for v in t) >= FR.N_EACH_SIDE
        if op == FR.OP_MUL_LAZY:
            assert p in t                                        # b = p with a non-zero a: exactly p, not reduced
        if op == FR.OP_MUL:                                      # both orders of the wide operand
            assert any(a >= p for a in a_rows) and any(b >= p for b in b_rows)
    for op in (FR.OP_DOT2, FR.OP_DOT4):
        if f.has(op):
            a_rows, b_rows = FR.operands(name, op)
            t = [FR.lazy(f, sum(x * y for x, y in zip(a, b))) for a, b in zip(a_rows, b_rows)]
            assert all(v < 2 * p for v in t) and p in t and any(v > p for v in t)
            assert any(p in a for a in a_rows) and any(p in b for b in b_rows)
    a_rows, b_rows = FR.operands(name, FR.OP_ADD)
    assert {p - 1, p, p + 1} <= {a + b for a, b in zip(a_rows, b_rows)}
    a_rows, b_rows = FR.operands(name, FR.OP_SUB)
    d = {a - b for a, b in zip(a_rows, b_rows)}
    assert 0 in d and -1 in d and any(v > 0 for v in d) and any(a == b and a for a, b in zip(a_rows, b_rows))
    a_rows, b_rows = FR.operands(name, FR.OP_ADD2P_SUB_RAW)
    assert sum(b == a + 2 * p for a, b in zip(a_rows, b_rows)) >= 8
    assert any(b > a for a, b in zip(a_rows, b_rows)) and any(b < a for a, b in zip(a_rows, b_rows))
    a_rows, _ = FR.operands(name, FR.OP_NEG_RAW)
    assert p in a_rows and 0 in a_rows
    a_rows, _ = FR.operands(name, FR.OP_NEG_RAW_2P)
    assert 2 * p in a_rows and 0 in a_rows
    a_rows, _ = FR.operands(name, FR.OP_COND_SUB_P)
    assert {p - 1, p, p + 1, f.R - 1} <= set(a_rows)
    a_rows, _ = FR.operands(name, FR.OP_REDUCE_FULL)
    if f is FR.STARK252:
        borrow, others = FR.stark_reduction_inputs()
        assert len(borrow) == 93 and len(others) == 32 + 62 and set(borrow + others) <= set(a_rows)
        assert {a >> 251 for a in a_rows} == set(range(32))
        for x in borrow:                                         # the quotient estimate is one too large: the + p fires
            assert x - (x >> 251) * p < 0 and x // p == (x >> 251) - 1
        for x in others:
            assert x - (x >> 251) * p >= 0
    else:
        assert {p - 1, p, p + 1, 2 * p - 1} <= set(a_rows) and max(a_rows) < 2 * p


def test_babybear_vector_sets_meet_their_coverage_conditions():
    p = FR.BB_P
    a, _ = FR.bb_operands(FR.OP_REDUCE64)
    assert {0, (p - 1) ** 2, 2 * (p - 1) ** 2, p * FR.BB_R - 1} <= set(a) and max(a) == p * FR.BB_R - 1
    raw = [FR.bb_reduce_raw(x) for x in a]
    assert all(r < 2 * p for r in raw)
    assert sum(r >= p for r in raw) >= 16 and sum(r < p for r in raw) >= 16      # both outcomes of the final min
    assert p in raw or p - 1 in raw
    for op in (FR.OP_ADD, FR.OP_SUB, FR.OP_MUL):
        a, b = FR.bb_operands(op)
        assert len(a) == len(FR.bb_words()) ** 2 + FR.N_RANDOM
    a, b = FR.bb_operands(FR.OP_ADD)
    assert {p - 1, p, p + 1, 2 * p - 2} <= {x + y for x, y in zip(a, b)}
    a, b = FR.bb_operands(FR.OP_SUB)
    assert {0, -1, 1, 1 - p, p - 1} <= {x - y for x, y in zip(a, b)}
