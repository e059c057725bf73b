"""The scalar-operand columns FusedColS<Stark252, K> (tools/gen_mac_chains.py, a_sgpr) are the a < p columns with a's limbs
as the MACs' scalar operand, for a twiddle shared by a whole wavefront (fe_mul_lazy_uniform).

The interval model of tests/test_mac_chain_bounds_cpu.py does not depend on the register class of an operand, so the proof
carries over if and only if the emitted statements are the same MACs in the same order with the same add-with-carry
pattern.  This parses the emitted text and checks exactly that, runs the whole product through the same interpreter
against big-integer Montgomery on the extremes the bounds rest on, and checks what the variant adds: every a limb is
an "s" operand and no v_mad_u64_u32 has more than one scalar operand (the constant-bus limit of the instruction)."""
import re

from tests import test_mac_chain_bounds_cpu as B
from tools import gen_mac_chains as G

P, N = B.P, B.N


def sgpr_text(k):
    return G.fused_col("Stark252", P, k, a_canonical=True, a_sgpr=True)


S_COLS = [B.parse_column(sgpr_text(k)) for k in range(2 * N - 1)]


def test_same_macs_same_order_same_carries_as_the_a_lt_p_columns():
    for k in range(2 * N - 1):
        assert S_COLS[k] == B.COLS[True][k], k
        plan = G.fused_col_plan(P, k, True)
        assert len([i for i in S_COLS[k] if i[0] == "mad"]) == len(plan["macs"])


def test_product_through_the_scalar_columns_matches_big_integer_montgomery(monkeypatch):
    monkeypatch.setitem(B.COLS, True, S_COLS)
    for a, b in B.in_contract_cases():
        got, lost = B.model_product(a, b, True)
        assert not lost, (hex(a), hex(b))
        assert got == B.montgomery(a, b), (hex(a), hex(b))
        if a < B.P_INT:
            assert got < 2 * B.P_INT


def test_a_is_the_only_scalar_register_operand_and_each_mac_has_at_most_one():
    for k in range(2 * N - 1):
        text = sgpr_text(k)
        outs, ins, _ = [ln.strip()[1:] for ln in text.splitlines() if ln.strip().startswith(":")]
        cons = re.findall(r'"([=&+vs]+)"\(((?:[^()]|\([^()]*\))*)\)', outs + "," + ins)
        for c, expr in cons:
            if expr.startswith("a.v["):
                assert c == "s", (k, expr)
            elif expr.startswith("Stark252::p("):
                assert c == "s", (k, expr)
            else:
                assert "s" not in c, (k, expr)          # lo, hi, init, b and m live in vector registers
        scalar = [c == "s" for c, _ in cons]
        for ins_text in re.findall(r'"(v_mad_u64_u32[^"\\]*)', text):
            args = [s.strip() for s in ins_text.split(None, 1)[1].split(",")]
            srcs = args[2:5]
            n_scalar = sum(1 for t in srcs if t.startswith("%") and scalar[int(t[1:])])
            assert n_scalar <= 1, (k, ins_text)
            # an inline constant (p's 17) is not a scalar register and may sit next to a vector operand only
            if any(not t.startswith("%") and t != "0" for t in srcs[:2]):
                assert n_scalar == 0, (k, ins_text)


def test_general_and_a_lt_p_columns_are_unchanged_by_the_variant():
    for k in range(2 * N - 1):
        for a_lt_p in (False, True):
            assert '"s"(a.v[' not in G.fused_col("Stark252", P, k, a_canonical=a_lt_p)


def test_committed_file_has_the_scalar_columns():
    text = open(G.output_path()).read()
    for k in range(2 * N - 1):
        assert f"struct FusedColS<Stark252, {k}>" in text
        assert sgpr_text(k) in text
