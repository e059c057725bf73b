#!/usr/bin/env python3
"""Generates lambda_elliptic_curves_amd/csrc/mac_chains.inc: one inline-asm statement per Montgomery column.

hipcc pads one wait state after every asm statement, so a column written as several short MAC statements pays a
s_nop per statement.  This emits, for every product count n = 1..12, a function whose single statement starts the
column (first MAC takes the previous column's carry as addend) and chains the remaining a*b MACs, and one that
chains n m*p MACs with the modulus limbs as SGPR literals.  For the fields in FUSED_FIELDS it also emits, per column,
one statement holding all of the column's a*b and m*p MACs with the sparse modulus compiled in."""
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


def fused_col(field, p, k):
    """Column k of a*b + m*p as one statement: lo(64) / hi(32) = init + sum a[i]*b[k-i] + sum m[i]*p[k-i] over every
    MAC of the column except the unit limb's m[k]*p[0] (lw_redc_unit in field.cuh does that one without a multiply).

    The reduction MACs go first.  A column's addend is (previous column) >> 64 < 2^40: each column sums at most
    2N - 2 + 2 products below 2^64, so its top word is small.  While the running sum provably stays below 2^64 (the
    addend, then m*p[j] < 2^32 * p[j] for the small limbs of a sparse modulus, or a*b alone in column 0) a MAC cannot
    carry out of the low pair, so it needs no add-with-carry; the top word starts on the first MAC that can carry.
    The top word of the last column is never read (the result fits N limbs), so that column has no add-with-carry."""
    n = len(p)
    assert p[0] == 1
    last = 2 * n - 2
    mp = [(i, k - i) for i in range(max(0, k - n + 1), min(k, n)) if p[k - i] != 0]
    ab = [(i, k - i) for i in range(max(0, k - n + 1), min(k, n - 1) + 1)]
    # how many leading MACs cannot carry
    bound = (1 << 40) if k > 0 else 0
    safe = 0
    for _, j in mp:
        bound += p[j] << 32
        if bound >= 1 << 64:
            break
        safe += 1
    if safe == len(mp) and ab and bound + ((1 << 32) - 1) ** 2 < (1 << 64):
        safe += 1                         # column 0: a[0]*b[0] with no addend
    # outputs: %0 lo, %1 hi (none in the last column, nor in a column whose MACs cannot carry: its top word is 0)
    has_hi = k != last and safe < len(mp) + len(ab)
    ins, macs = [], []
    opn = 2 if has_hi else 1
    init = None
    if k > 0:
        init = f"%{opn}"
        ins.append('"v"(init)')
        opn += 1
    for i, j in mp:
        if p[j] <= 64:                    # inline constant
            macs.append((f"%{opn}", str(p[j])))
            ins.append(f'"v"(m[{i}])')
            opn += 1
        else:                             # SGPR literal
            macs.append((f"%{opn}", f"%{opn + 1}"))
            ins.append(f'"v"(m[{i}])')
            ins.append(f'"s"({field}::p({j}))')
            opn += 2
    for i, j in ab:
        macs.append((f"%{opn}", f"%{opn + 1}"))
        ins.append(f'"v"(a.v[{i}])')
        ins.append(f'"v"(b.v[{j}])')
        opn += 2
    body, hi_live = [], False
    for q, (x, y) in enumerate(macs):
        addend = "%0" if q > 0 else (init or "0")
        body.append(f'"v_mad_u64_u32 %0, vcc, {x}, {y}, {addend}\\n\\t"')
        if not has_hi or q < safe:
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
    sep = "\n            "
    return (f"template <>\n"
            f"struct FusedCol<{field}, {k}> {{   // {len(ab)} a*b + {len(mp)} m*p MACs\n"
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
    out = [f"// {field}: the whole product, one statement per column (FusedCol<F, K>::run, used by fips_fused)\n"
           f"static_assert({field}::N == {n} && {checks}, \"modulus changed: rerun tools/gen_mac_chains.py\");\n"
           f"template <>\nstruct lw_fused_columns<{field}> {{\n    static constexpr bool value = true;\n}};\n"]
    for k in range(2 * n - 1):
        out.append(fused_col(field, p, k))
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
