#!/usr/bin/env python3
"""Generates lambda_elliptic_curves_amd/csrc/mac_chains.inc: one inline-asm statement per Montgomery column.

hipcc pads one wait state after every asm statement, so a column written as several short MAC statements pays a
s_nop per statement.  This emits, for every product count n = 1..12, a function whose single statement starts the
column (first MAC takes the previous column's carry as addend) and chains the remaining a*b MACs, and one that
chains n m*p MACs with the modulus limbs as SGPR literals.  For the fields in FUSED_FIELDS it also emits, per column,
one statement holding all of the column's a*b and m*p MACs with the sparse modulus compiled in.

A MAC needs an add-with-carry into the column's top word only if the 64-bit running sum can overflow.  fused_col_plan
proves per column, by exact interval arithmetic over per-limb operand bounds, which leading MACs cannot: (1) the carry into
column K is at most floor(S_{K-1} / 2^32) for the previous column's largest sum S, unit limb included, which spares the
first a*b MAC of columns 1 and 2 for any operands; (2) for callers that promise a < p (precondition of the A_LT_P = true
columns, used by fe_mul_lazy only) a's top limb is at most p's, so in Stark252's columns 7 to 13 a[7]*b[K-7] goes right
behind the two m*p MACs and needs none either.  Every bound is asserted below 2^64 when the file is generated."""
MAC = 'LW_MAC_V("%{a}", "%{b}")'


def col_ab_first(n):
    # operands: %0 lo (out), %1 hi (out), %2 init, then a0,b0,a1,b1,...
    ops = []
    body = ['LW_MAC_FIRST("%3", "%4", "%2")']
    for j in range(1, n):
        body.append(MAC.format(a=3 + 2 * j, b=4 + 2 * j))
    ins = ['"v"(init)']
    for j in range(n):
        ins.append(f'"v"(a.v[I + {j}])')
        ins.append(f'"v"(b.v[K - I - {j}])')
    early = "=&v" if n > 1 else "=v"
    return (f"template <class F, int K, int I>\n"
            f"__device__ __forceinline__ void col_ab_first_n{n}(uint64_t &lo, uint32_t &hi, uint64_t init, const Fe<F> &a, const Fe<F> &b) {{\n"
            f"    asm({' '.join(body)}\n        : \"{early}\"(lo), \"{early}\"(hi)\n        : {', '.join(ins)}\n        : \"vcc\");\n}}\n")


def col_mp(n):
    # operands: %0 lo (+), %1 hi (+), then m0,c0,m1,c1,...   (c = SGPR literal)
    body = [MAC.format(a=2 + 2 * j, b=3 + 2 * j) for j in range(n)]
    ins = []
    for j in range(n):
        ins.append(f'"v"(m[I + {j}])')
        ins.append(f'"s"(F::p(K - I - {j}))')
    return (f"template <class F, int K, int I>\n"
            f"__device__ __forceinline__ void col_mp_n{n}(uint64_t &lo, uint32_t &hi, const uint32_t (&m)[F::N]) {{\n"
            f"    asm({' '.join(body)}\n        : \"+v\"(lo), \"+v\"(hi)\n        : {', '.join(ins)}\n        : \"vcc\");\n}}\n")


def dispatch(name, args, maxn, extra=""):
    lines = [f"template <class F, int K, int I, int CNT>\n__device__ __forceinline__ void {name}_dispatch({args}) {{"]
    for n in range(1, maxn + 1):
        kw = "if" if n == 1 else "else if"
        call = f"{name}_n{n}<F, K, I>({extra});"
        lines.append(f"    {kw} constexpr (CNT == {n}) {call}")
    lines.append('    else static_assert(CNT >= 1 && CNT <= %d, "unsupported MAC count");' % maxn)
    lines.append("}\n")
    return "\n".join(lines)


# Fields that get one fused statement per column of the whole product: 32-bit modulus limbs, least significant first.
# Only moduli with p = 1 mod 2^32 (so INV = -1 and m_k = -t_k) qualify: fips_fused in field.cuh reduces the unit limb
# without a multiplication.  The output checks these limbs against field.cuh with a static_assert.
FUSED_FIELDS = {
    "Stark252": [0x00000001, 0, 0, 0, 0, 0, 0x00000011, 0x08000000],
}


W = (1 << 32) - 1          # largest 32-bit word


def operand_bounds(p, a_canonical):
    """Largest value of every limb of a, b and m.  b and m are arbitrary words.  a is arbitrary too, unless the caller
    promises a < p (a_canonical): then its top limb is at most p's top limb (the lower limbs stay arbitrary)."""
    n = len(p)
    a = [W] * n
    if a_canonical:
        a[n - 1] = p[n - 1]
    return a, [W] * n, [W] * n


def fused_col_plan(p, k, a_canonical=False):
    """Column k of a*b + m*p as a list of MACs in issue order, with the proof that the carry-less ones cannot carry.

    -> dict(macs=[(kind, i, j, carry)], has_hi, carry_in, proof=[(q, bound)], total)
       kind 'mp': m[i]*p[j], 'ab': a[i]*b[j]; carry: an add-with-carry into the top word follows this MAC;
       carry_in: largest addend the previous column can hand over; proof: for every carry-less MAC q the largest value
       the 64-bit running sum can have after it (asserted below 2^64); total: the column's largest sum, unit limb included.

    Interval arithmetic, exact (no rounding up: column 2's first MAC reaches 2^64 - 1):
      * the carry into column k is floor(S / 2^32) of the largest sum S of column k - 1, where S includes the unit
        limb's m[k-1] <= 2^32 - 1 (lw_redc_unit adds it before the shift).  Column 0 hands over <= 2^32 - 1 and column 1
        <= 2^33 - 2, so the first a*b MAC of columns 1 and 2 cannot carry: (2^32 - 1)^2 + 2^33 - 2 = 2^64 - 1.
      * a MAC is bounded by the product of its operands' bounds: m[i]*p[j] <= (2^32 - 1)*p[j], and with a < p
        (a_canonical) a[N-1]*b[j] <= p[N-1]*(2^32 - 1), below 2^59 for Stark252.
    The reduction MACs go first, then the a*b MACs smallest bound first (a stable sort: with equal bounds the order is
    i ascending), and the top word starts on the first MAC whose running bound reaches 2^64.  The top word of the last
    column is never read (the result fits N limbs), so that column has no add-with-carry."""
    n = len(p)
    assert p[0] == 1
    last = 2 * n - 2
    amax, bmax, mmax = operand_bounds(p, a_canonical)
    carry_in = 0
    if k > 0:
        carry_in = fused_col_plan(p, k - 1, a_canonical)["total"] >> 32
    mp = [("mp", i, k - i, mmax[i] * p[k - i]) for i in range(max(0, k - n + 1), min(k, n)) if p[k - i] != 0]
    ab = [("ab", i, k - i, amax[i] * bmax[k - i]) for i in range(max(0, k - n + 1), min(k, n - 1) + 1)]
    ab.sort(key=lambda t: t[3])
    order = mp + ab
    # how many leading MACs cannot carry
    bound, safe, proof = carry_in, 0, []
    for q, (_, _, _, mx) in enumerate(order):
        if bound + mx >= 1 << 64:
            break
        bound += mx
        proof.append((q, bound))
        safe += 1
    for q, b in proof:
        assert b < 1 << 64, (k, q, hex(b))
    # none in the last column, nor in a column whose MACs cannot carry: its top word is 0
    has_hi = k != last and safe < len(order)
    total = carry_in + sum(t[3] for t in order) + (mmax[k] * p[0] if k < n else 0)
    # the 96-bit accumulator holds every column; the last column's sum must fit the low pair since its top word is dropped
    assert total < 1 << 96 and (k != last or not a_canonical or total < 1 << 64), (k, hex(total))
    macs = [(kind, i, j, has_hi and q >= safe) for q, (kind, i, j, _) in enumerate(order)]
    return dict(macs=macs, has_hi=has_hi, carry_in=carry_in, proof=proof, total=total)


def fused_col(field, p, k, a_canonical=False, a_sgpr=False):
    """Column k of a*b + m*p as one statement: lo(64) / hi(32) = init + sum a[i]*b[k-i] + sum m[i]*p[k-i] over every
    MAC of the column except the unit limb's m[k]*p[0] (lw_redc_unit in field.cuh does that one without a multiply).
    Which MACs carry an add-with-carry, and why the others need none, is fused_col_plan's business.

    a_canonical: the variant FusedCol<F, K, true> for callers whose contract says a < p (fe_mul_lazy: the NTT's
    twiddles and scale factors).  Where the bound on a's top limb changes nothing it inherits the general column.

    a_sgpr: the variant FusedColS<F, K> of the a < p columns for an a that is the same in every lane of the wavefront
    (a twiddle shared by a whole wave): its limbs are the MACs' scalar operand, as p's limbs are in the m*p MACs (one
    scalar operand per v_mad_u64_u32), so a occupies no vector registers.  Same MACs in the same order with the same
    add-with-carry pattern as FusedCol<F, K, true>: the bounds do not depend on where an operand lives."""
    n = len(p)
    last = 2 * n - 2
    assert a_canonical or not a_sgpr
    plan = fused_col_plan(p, k, a_canonical)
    if a_canonical and not a_sgpr and plan["macs"] == fused_col_plan(p, k, False)["macs"]:
        return (f"template <>\n"
                f"struct FusedCol<{field}, {k}, true> : FusedCol<{field}, {k}, false> {{}};   // a < p changes nothing here\n")
    has_hi = plan["has_hi"]
    nab = sum(1 for m in plan["macs"] if m[0] == "ab")
    nmp = len(plan["macs"]) - nab
    ins, macs = [], []
    opn = 2 if has_hi else 1
    init = None
    if k > 0:
        init = f"%{opn}"
        ins.append('"v"(init)')
        opn += 1
    for kind, i, j, _ in plan["macs"]:
        if kind == "mp" and p[j] <= 64:   # inline constant
            macs.append((f"%{opn}", str(p[j])))
            ins.append(f'"v"(m[{i}])')
            opn += 1
        elif kind == "mp":                # SGPR literal
            macs.append((f"%{opn}", f"%{opn + 1}"))
            ins.append(f'"v"(m[{i}])')
            ins.append(f'"s"({field}::p({j}))')
            opn += 2
        else:
            macs.append((f"%{opn}", f"%{opn + 1}"))
            ins.append(f'"{"s" if a_sgpr else "v"}"(a.v[{i}])')
            ins.append(f'"v"(b.v[{j}])')
            opn += 2
    body, hi_live = [], False
    for q, (x, y) in enumerate(macs):
        addend = "%0" if q > 0 else (init or "0")
        body.append(f'"v_mad_u64_u32 %0, vcc, {x}, {y}, {addend}\\n\\t"')
        if not plan["macs"][q][3]:
            continue
        if hi_live:
            body.append('"v_addc_co_u32_e32 %1, vcc, 0, %1, vcc\\n\\t"')
        else:
            body.append('"v_addc_co_u32_e64 %1, vcc, 0, 0, vcc\\n\\t"')
            hi_live = True
    early = "=&v" if len(macs) > 1 else "=v"
    outs = [f'"{early}"(lo)'] + ([f'"{early}"(hi)'] if has_hi else [])
    if k == last:
        tail = "        hi = 0;   // the top word of the last column is zero and never computed\n"
    elif not has_hi:
        tail = "        hi = 0;\n"
    else:
        tail = ""
    if plan["proof"]:
        q, b = plan["proof"][-1]
        why = f"    // addend <= 0x{plan['carry_in']:x}; no carry out of the low pair up to MAC {q}: sum <= 0x{b:x}\n"
    else:
        why = f"    // addend <= 0x{plan['carry_in']:x}; every MAC can carry\n"
    sep = "\n            "
    name = f"FusedColS<{field}, {k}>" if a_sgpr else f"FusedCol<{field}, {k}, {'true' if a_canonical else 'false'}>"
    return (f"template <>\n"
            f"struct {name} {{   // {nab} a*b + {nmp} m*p MACs\n"
            f"{why}"
            f"    __device__ static __forceinline__ void run(uint64_t &lo, uint32_t &hi, uint64_t init, const Fe<{field}> &a, "
            f"const Fe<{field}> &b, const uint32_t (&m)[{n}]) {{\n"
            f"        asm({sep.join(body)}\n"
            f"            : {', '.join(outs)}\n"
            f"            : {', '.join(ins)}\n"
            f"            : \"vcc\");\n"
            f"{tail}"
            f"    }}\n}};\n")


def fused_field(field, p):
    n = len(p)
    checks = " && ".join(f"{field}::p({i}) == 0x{v:08x}u" for i, v in enumerate(p))
    out = [f"// {field}: the whole product, one statement per column (FusedCol<F, K, A_LT_P>::run, used by fips_fused).\n"
           f"// A_LT_P = true is for callers that promise a < p: a[{n - 1}] <= 0x{p[n - 1]:x} spares one add-with-carry in the columns it is in.\n"
           f"static_assert({field}::N == {n} && {checks}, \"modulus changed: rerun tools/gen_mac_chains.py\");\n"
           f"template <>\nstruct lw_fused_columns<{field}> {{\n    static constexpr bool value = true;\n}};\n"]
    for k in range(2 * n - 1):
        out.append(fused_col(field, p, k))
    for k in range(2 * n - 1):
        out.append(fused_col(field, p, k, a_canonical=True))
    out.append(f"// {field}: the a < p columns for a wave-uniform a, whose limbs are the scalar operand of the a*b MACs (fips_fused, A_SGPR).\n")
    for k in range(2 * n - 1):
        out.append(fused_col(field, p, k, a_canonical=True, a_sgpr=True))
    return out


def render():
    out = ["// GENERATED by tools/gen_mac_chains.py — do not edit.  Whole-column MAC chains (see field.cuh).\n"]
    for n in range(1, 13):
        out.append(col_ab_first(n))
    for n in range(1, 12):
        out.append(col_mp(n))
    out.append(dispatch("col_ab_first", "uint64_t &lo, uint32_t &hi, uint64_t init, const Fe<F> &a, const Fe<F> &b", 12, "lo, hi, init, a, b"))
    out.append(dispatch("col_mp", "uint64_t &lo, uint32_t &hi, const uint32_t (&m)[F::N]", 11, "lo, hi, m"))
    for field, p in FUSED_FIELDS.items():
        out.extend(fused_field(field, p))
    return "\n".join(out)


def output_path():
    import os
    return os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "lambda_elliptic_curves_amd", "csrc", "mac_chains.inc")


def main():
    path = output_path()
    open(path, "w").write(render())
    print("wrote", path)


if __name__ == "__main__":
    main()
