"""The carry adds that tools/gen_mac_chains.py leaves out of the fused Stark252 columns are provably zero.

A wrong bound would be a silent wrong product for rare operands, so this does not sample the device: it parses the column
statements the generator emits (the text of mac_chains.inc) and interprets them with the hardware's semantics: a 64-bit
low pair that wraps, v_mad_u64_u32 setting vcc to the carry out of it, and a top word that only changes where a
v_addc_co_u32 was emitted.  The whole product, chained through the unit-limb step exactly as fips_fused does, is then
compared with big-integer Montgomery on the extremes the bounds rest on, and the model is shown to bite: outside the
a < p precondition the A_LT_P columns do come out wrong."""
import random
import re

import pytest

from tools import gen_mac_chains as G

P = G.FUSED_FIELDS["Stark252"]
N = len(P)
M32, M64 = (1 << 32) - 1, (1 << 64) - 1
R = 1 << (32 * N)
P_INT = sum(v << (32 * i) for i, v in enumerate(P))
P_INV = pow(P_INT, -1, R)


def limbs(x):
    return [(x >> (32 * i)) & M32 for i in range(N)]


def parse_column(text):
    """-> list of ('mad', x, y, addend) / ('addc64',) / ('addc32',) with operands as ('lo',), ('hi',), ('init',),
    ('a', i), ('b', j), ('m', i), ('p', j) or ('imm', value)"""
    body = re.findall(r'"(v_[^"\\]*)', text)
    outs, ins, _ = [ln.strip()[1:] for ln in text.splitlines() if ln.strip().startswith(":")]
    ops = []
    for expr in re.findall(r'"[=&+vs]+"\(((?:[^()]|\([^()]*\))*)\)', outs + "," + ins):
        m = re.fullmatch(r"(lo|hi|init)", expr)
        if m:
            ops.append((expr,))
            continue
        m = re.fullmatch(r"(a|b)\.v\[(\d+)\]", expr) or re.fullmatch(r"(m)\[(\d+)\]", expr) or re.fullmatch(r"Stark252::(p)\((\d+)\)", expr)
        assert m, expr
        ops.append((m.group(1), int(m.group(2))))

    def operand(tok):
        return ops[int(tok[1:])] if tok.startswith("%") else ("imm", int(tok))

    prog = []
    for ins_text in body:
        name, rest = ins_text.split(None, 1)
        args = [s.strip() for s in rest.split(",")]
        if name == "v_mad_u64_u32":
            assert args[0] == "%0" and args[1] == "vcc"
            prog.append(("mad", operand(args[2]), operand(args[3]), operand(args[4])))
        elif name == "v_addc_co_u32_e64":
            assert args == ["%1", "vcc", "0", "0", "vcc"] and ops[1] == ("hi",)
            prog.append(("addc64",))
        elif name == "v_addc_co_u32_e32":
            assert args == ["%1", "vcc", "0", "%1", "vcc"] and ops[1] == ("hi",)
            prog.append(("addc32",))
        else:
            raise AssertionError(ins_text)
    return prog


def columns(a_lt_p):
    cols = []
    for k in range(2 * N - 1):
        text = G.fused_col("Stark252", P, k, a_canonical=a_lt_p)
        if "asm(" not in text:                      # inherits the general column
            assert a_lt_p and f": FusedCol<Stark252, {k}, false>" in text
            text = G.fused_col("Stark252", P, k)
        cols.append(parse_column(text))
    return cols


COLS = {False: columns(False), True: columns(True)}


def run_column(prog, init, a, b, m):
    """-> lo, hi, lost: lost = some MAC carried out of the low pair with no add-with-carry behind it"""
    env = {"init": init, "lo": None, "hi": 0}        # hi = 0 is what run() assigns where no top word is computed
    vcc, lost = 0, False

    def val(op):
        if op[0] == "imm":
            return op[1]
        if op[0] in env:
            return env[op[0]]
        return {"a": a, "b": b, "m": m, "p": P}[op[0]][op[1]]

    for q, ins in enumerate(prog):
        if ins[0] == "mad":
            s = val(ins[1]) * val(ins[2]) + val(ins[3])
            env["lo"], vcc = s & M64, s >> 64
            assert vcc <= 1
            if vcc and (q + 1 == len(prog) or prog[q + 1][0] == "mad"):
                lost = True
        elif ins[0] == "addc64":
            env["hi"] = vcc
            vcc = 0
        else:
            s = env["hi"] + vcc
            env["hi"], vcc = s & M32, s >> 32
    return env["lo"], env["hi"], lost


def model_product(a_int, b_int, a_lt_p):
    """fips_fused<Stark252, 0, a_lt_p>: -> (t as an integer, lost), lost ignoring the last column, whose top word is
    dropped on purpose"""
    a, b = limbs(a_int), limbs(b_int)
    m, t, init, lost_any = [0] * N, [0] * N, 0, False
    for k, prog in enumerate(COLS[a_lt_p]):
        lo, hi, lost = run_column(prog, init, a, b, m)
        if k != 2 * N - 2:
            lost_any |= lost
        if k < N:                                     # lw_redc_unit / lw_redc_unit0
            tk, w1 = lo & M32, lo >> 32
            m[k] = (-tk) & M32
            s = w1 + (1 if tk else 0)
            mid, c = s & M32, s >> 32
            top = (hi + c) & M32
            init = (top << 32) | mid
        else:
            t[k - N] = lo & M32
            init = ((lo >> 32) | (hi << 32)) & M64
    t[N - 1] = init & M32
    return sum(v << (32 * i) for i, v in enumerate(t)), lost_any


def montgomery(a_int, b_int):
    ab = a_int * b_int
    m = (-ab * P_INV) % R
    q, rem = divmod(ab + m * P_INT, R)
    assert rem == 0
    return q


ONES = R - 1
A_EXTREME = (1 << 27 << 224) | ((1 << 224) - 1)      # a[7] = 2^27, every lower limb 0xffffffff: the bound's extreme (> p)


def low_ones(k):
    return (1 << (32 * (k + 1))) - 1


def in_contract_cases():
    a_set = [0, 1, P_INT - 1, A_EXTREME, (1 << 251) - 1, 1 << 251, P_INT - 2, low_ones(6), (1 << 27) << 224]
    b_set = [0, 1, ONES, P_INT - 1, A_EXTREME, low_ones(0), low_ones(1), low_ones(2), ONES - 1, ONES ^ 1, ONES ^ (1 << 32)]
    cases = [(a, b) for a in a_set for b in b_set]
    # operands that maximise the carry into every column: all-ones limbs up to k, and a's top limb at its bound
    for ka in range(N):
        for kb in range(N):
            a = low_ones(ka) if ka < N - 1 else A_EXTREME
            cases.append((a, low_ones(kb)))
            cases.append((a, ONES ^ low_ones(kb) if kb < N - 1 else ONES))
    rng = random.Random(252)
    for _ in range(3000):
        cases.append((rng.randrange(P_INT), rng.randrange(R)))
    for _ in range(1000):                             # a's top limb pinned at the bound, b dense in ones
        a = ((1 << 27) << 224) | rng.randrange(1 << 224)
        cases.append((a, ONES ^ (1 << rng.randrange(256))))
    return cases


def test_a_lt_p_columns_match_big_integer_montgomery():
    for a, b in in_contract_cases():
        got, lost = model_product(a, b, True)
        exp = montgomery(a, b)
        assert not lost, (hex(a), hex(b))
        assert exp < R and got == exp, (hex(a), hex(b))
        if a < P_INT:
            assert got < 2 * P_INT


def test_general_columns_match_for_any_operands():
    rng = random.Random(253)
    cases = in_contract_cases()
    cases += [(ONES, ONES), (ONES, 1), (ONES, P_INT - 1), (ONES ^ 1, ONES), (low_ones(2), ONES), (ONES, low_ones(2))]
    cases += [(rng.randrange(R), rng.randrange(R)) for _ in range(3000)]
    for a, b in cases:
        got, lost = model_product(a, b, False)
        assert not lost, (hex(a), hex(b))
        assert got == montgomery(a, b) % R, (hex(a), hex(b))   # above 2^256 only when a is far above p


def test_tight_bound_of_columns_1_and_2_is_reached():
    # all-ones operands drive the addend of column 1 to 2^32 - 1 and of column 2 to 2^33 - 2, and the first MAC of
    # column 2 to 2^64 - 1 exactly: the bound is attained, not merely approached, and still does not carry
    a, b, m, init = limbs(ONES), limbs(ONES), [0] * N, 0
    seen = []
    for k in range(3):
        seen.append(init)
        lo, hi, lost = run_column(COLS[False][k], init, a, b, m)
        assert not lost
        tk = lo & M32
        m[k] = (-tk) & M32
        init = ((lo + (hi << 64) + m[k]) >> 32) & M64
    assert seen == [0, (1 << 32) - 1, (1 << 33) - 2]
    assert a[0] * b[2] + seen[2] == M64


def test_model_bites_outside_the_precondition():
    # a[7] = 0xffffffff breaks a < p: the A_LT_P columns drop a carry that happens, and the product is wrong
    got, lost = model_product(ONES, ONES, True)
    assert lost
    assert got != montgomery(ONES, ONES) % R
    got, lost = model_product(ONES, ONES, False)
    assert not lost and got == montgomery(ONES, ONES) % R


@pytest.mark.parametrize("a_lt_p", [False, True])
def test_generator_proof_holds_and_matches_the_emitted_text(a_lt_p):
    # recompute every bound from scratch: largest addend, then each carry-less MAC's running sum
    amax = [M32] * (N - 1) + [P[N - 1] if a_lt_p else M32]
    carry_in, addc = 0, 0
    for k, prog in enumerate(COLS[a_lt_p]):
        plan = G.fused_col_plan(P, k, a_lt_p)
        assert plan["carry_in"] == carry_in
        for _, bound in plan["proof"]:
            assert bound < 1 << 64
        mads = [i for i in prog if i[0] == "mad"]
        assert len(mads) == len(plan["macs"])
        running, total, q = carry_in, carry_in, 0
        for idx, ins in enumerate(prog):
            if ins[0] != "mad":
                addc += 1
                continue
            x, y = ins[1], ins[2]
            if x[0] == "m":
                mx = M32 * (y[1] if y[0] == "imm" else P[y[1]])
                assert plan["macs"][q][:3] == ("mp", x[1], k - x[1])
            else:
                assert x[0] == "a" and y[0] == "b" and x[1] + y[1] == k
                mx = amax[x[1]] * M32
                assert plan["macs"][q][:3] == ("ab", x[1], y[1])
            total += mx
            carries = idx + 1 < len(prog) and prog[idx + 1][0] != "mad"
            assert carries == plan["macs"][q][3]
            if not carries and k != 2 * N - 2:
                running += mx
                assert running < 1 << 64, (k, q, hex(running))
                assert all(p[0] == "mad" for p in prog[:idx]), "carry-less MACs lead the column"
            q += 1
        if k < N:
            total += M32                              # the unit limb's m[k]*p[0]
        assert total == plan["total"]
        carry_in = total >> 32
    # 62 before the exact bounds: 2 fewer for any operands (columns 1 and 2), 7 more with a < p (columns 7 to 13)
    assert addc == (53 if a_lt_p else 60)


def test_committed_file_has_both_variants():
    text = open(G.output_path()).read()
    for k in range(2 * N - 1):
        assert f"struct FusedCol<Stark252, {k}, false>" in text and f"struct FusedCol<Stark252, {k}, true>" in text
