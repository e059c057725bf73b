"""Static budget of the ntt_pass_kernel instances from gfx950 assembly (the tables of profiles/ntt_*_isa.txt).

    hipcc -O3 -std=c++17 --offload-arch=gfx950 --cuda-device-only -S lambda_elliptic_curves_amd/csrc/ntt256.hip -o ntt256.s
    python tools/ntt_isa_table.py ntt256.s [Stark252|Fr381] [fx ...]

Counts are static, per work-item: instructions between a kernel's label and its s_endpgm, and the compiler's kernel
info block behind it (vgpr = NumVgprs, scratch = ScratchSize, lds = LDSByteSize, waves/SIMD = Occupancy).
"""
import re
import sys

COLS = [("v_mad_u64_u32", r"v_mad_u64_u32"), ("addc_e32", r"v_addc_co_u32_e32"), ("addc_e64", r"v_addc_co_u32_e64"),
        ("v_sub*", r"v_sub"), ("v_mov", r"v_mov_b32"), ("s_nop", r"s_nop"), ("valu", r"v_(?!_)"),
        ("ds_r128", r"ds_read_b128"), ("ds_w128", r"ds_write_b128"), ("g_load", r"global_load_dwordx4"),
        ("g_store", r"global_store_dwordx4"), ("s_barrier", r"s_barrier")]


def kernels(path):
    text = open(path).read()
    meta = {}
    for m in re.finditer(r"^(_Z\w+):", text, re.M):
        name = m.group(1)
        rest = text[m.end():]
        if "s_endpgm" not in rest:
            continue
        body, info = rest[:rest.index("s_endpgm")], rest[rest.index("s_endpgm"):]
        info = info[:info.index("; Occupancy:") + 40]
        ins = [ln.split()[0] for ln in body.splitlines() if ln.startswith("\t") and ln.strip() and not ln.lstrip().startswith((".", ";"))]
        field = lambda key: int(re.search(r"; %s: (\d+)" % key, info).group(1))
        meta[name] = {"vgpr": field("NumVgprs"), "scratch": field("ScratchSize"), "lds": field("LDSByteSize"), "waves": field("Occupancy"),
                      "counts": {c: sum(1 for i in ins if re.match(rx, i)) for c, rx in COLS}}
    return meta


def main():
    path, field = sys.argv[1], (sys.argv[2] if len(sys.argv) > 2 else "Stark252")
    fxs = [int(a) for a in sys.argv[3:]] or [8, 7, 6]
    rows = []
    for name, info in kernels(path).items():
        m = re.search(r"ntt_pass_kernelINS_\d+%sELb([01])ELb([01])ELb([01])ELi(\d)E" % field, name)
        if not m or int(m.group(4)) not in fxs:
            continue
        last, extra, wl, fx = (int(g) for g in m.groups())
        rows.append(((-fx, last, extra, wl), "last=%d extra=%d wl=%d fx=%d" % (last, extra, wl, fx), info))
    head = "%-28s" % "kernel" + "".join(" %13s" % c if c == "v_mad_u64_u32" else " %8s" % c for c, _ in COLS)
    print(head + " %5s %7s %6s %10s" % ("vgpr", "scratch", "lds", "waves/SIMD"))
    for _, label, info in sorted(rows):
        print("%-28s" % label + "".join((" %13d" if c == "v_mad_u64_u32" else " %8d") % info["counts"][c] for c, _ in COLS)
              + " %5d %7d %6d %10d" % (info["vgpr"], info["scratch"], info["lds"], info["waves"]))


if __name__ == "__main__":
    main()
