#!/usr/bin/env python3
"""The randomized AIR over Goldilocks with Fp2 and BabyBear with Fp4 (csrc/ext_aux.cuh, the _rap_ part of csrc/ext_round2.cuh),
trace 2^20, blow-up 4, every figure of a field taken in one process:
  aux      aux_fractions_device over the 2^20 trace rows, product and sum mode, four-term lists over four columns, next to
           torch's device-to-device copy of the bytes the call reads and writes (the columns twice, once per pass over the
           rows, and the D planes of the column once)
  rap      fibonacci_rap and read_only_memory through rap_constraint_evaluations_device, the z column an auxiliary column
           and the challenges in E, next to the same AIRs through constraint_evaluations_device with z a main column and the
           challenges in F (the code path that entry had before the RAP entry existed)
  all-F    the read-only-memory program with everything in F through both entries: the same arithmetic, once in
           ext_r2_transition_kernel and once in ext_r2_rap_transition_kernel
  kernels  device time of every kernel of the calls (lw_hip_profile_begin / end), a run of its own
  plonk    the three kernels of PLONK round 2's grand product (csrc/plonk.hip, BLS12-381 Fr, 2^20 rows: the same
           reduce-then-scan, there over 256-bit words with three-factor numerators and denominators) from the same kind of
           run in the same process, and the ratio of the product mode's three kernels to them, per row
Nothing but the all-F pair has an earlier measurement to be compared with.
Every step is a process of its own under `timeout -k 10`; the first step that fails or hangs ends the run.
usage: ext_rap_timing.py [--out FILE]        (ext_rap_timing.py --step NAME runs one step)"""
import argparse
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LOG_TRACE, LOG_BLOWUP = 20, 2
CALLS, SAMPLES = 10, 9
GL_P, BB_P = (1 << 64) - (1 << 32) + 1, 2013265921
STEPS = [("gl2", 400), ("bb4", 400)]


def timed(fn):
    """ms per call: SAMPLES samples of CALLS calls enqueued back to back, stream synchronised; median, min, max"""
    import torch
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(SAMPLES):
        t0 = time.perf_counter()
        for _ in range(CALLS):
            fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3 / CALLS)
    return statistics.median(out), min(out), max(out)


def fmt(t):
    return f"{t[0]:8.4f} ms [{t[1]:8.4f} .. {t[2]:8.4f}]"


def ratio(a, b):
    r = a[0] / b[0]
    return f"{r:.2f} +- {r * ((a[2] - a[1]) / (2 * a[0]) + (b[2] - b[1]) / (2 * b[0])):.2f}"


def programs(S):
    """name -> (with the challenges in F and z a main column, with the challenges in E and z an auxiliary column)"""
    one, z, alpha = S.const(0), S.const(1), S.const(2)
    step = S.cell(2, 1) - S.cell(2) - one
    rom = [(S.cell(2, 1) - S.cell(2)) * step, (S.cell(3, 1) - S.cell(3)) * step,
           (z - (S.cell(2, 1) + alpha * S.cell(3, 1))) * S.cell(4, 1) - (z - (S.cell(0, 1) + alpha * S.cell(1, 1))) * S.cell(4)]
    xz, xalpha = S.xconst(0), S.xconst(1)
    rom_rap = [(S.cell(2, 1) - S.cell(2)) * step, (S.cell(3, 1) - S.cell(3)) * step,
               (xz - (xalpha * S.cell(3, 1) + S.cell(2, 1))) * S.xcell(0, 1) - (xz - (xalpha * S.cell(1, 1) + S.cell(0, 1))) * S.xcell(0)]
    gamma, xgamma = S.const(0), S.xconst(0)
    fib = [S.cell(2, 1) * (S.cell(1) + gamma) - S.cell(2) * (S.cell(0) + gamma)]
    fib_rap = [S.xcell(0, 1) * (xgamma + S.cell(1)) - S.xcell(0) * (xgamma + S.cell(0))]
    return {"fib_rap": (fib, 3, 1, fib_rap, 2, 0, 1), "rom": (rom, 5, 3, rom_rap, 4, 1, 2)}


def step(field):
    import numpy as np
    import torch
    from lambda_elliptic_curves_amd import _lib, babybear_ext, goldilocks_ext, stark
    X, p, width, word_bytes, np_word, signed = ((goldilocks_ext, GL_P, 2, 8, np.uint64, np.int64) if field == "gl2" else
                                                (babybear_ext, BB_P, 4, 4, np.uint32, np.int32))
    n, N = 1 << LOG_TRACE, 1 << (LOG_TRACE + LOG_BLOWUP)
    rng = np.random.default_rng(1)
    column = lambda rows: torch.from_numpy(rng.integers(0, p, rows, dtype=np_word).view(signed)).cuda()
    scalar = lambda: tuple(int(v) for v in rng.integers(1, p, width, dtype=np_word))

    def copy_of(nbytes):
        src = torch.zeros(nbytes // 2, dtype=torch.uint8, device="cuda")
        dst = torch.empty_like(src)
        return timed(lambda: dst.copy_(src))

    calls = {}
    # ---- the auxiliary column
    trace = [column(n) for _ in range(4)]
    num, den = (scalar(), [(k, scalar()) for k in range(4)]), (scalar(), [(k, scalar()) for k in (1, 3, 0, 2)])
    t_aux = torch.empty(width * n, dtype=trace[0].dtype, device="cuda")
    moved = (2 * 4 + width) * n * word_bytes
    c = copy_of(moved)
    for label, mode in (("product", X.PRODUCT), ("sum", X.SUM)):
        call = lambda mode=mode: X.aux_fractions_device(trace, n, num, den, mode=mode, t_out=t_aux)
        calls[f"aux {label}"] = call
        t = timed(call)
        print(f"RESULT {field} aux {label:<8} four terms a side, 2^{LOG_TRACE} rows   call {fmt(t)}   copy of {moved / 2**20:6.1f} MiB moved {fmt(c)}   "
              f"call / copy = {ratio(t, c)}   {t[0] * 1e6 / n:.3f} ns per row")
    # ---- round 2
    cols = [column(N) for _ in range(5)]
    aux = [column(width * N)]
    t_out = torch.empty(width * N, dtype=cols[0].dtype, device="cuda")
    for air, (plain, n_cols, n_consts, rap, n_main, n_rap_consts, n_xconsts) in programs(stark).items():
        prog_plain, prog_rap = stark.compile_transitions(plain), stark.compile_transitions(rap)
        consts, xconsts = [int(v) for v in rng.integers(1, p, 3, dtype=np_word)], [scalar(), scalar()]
        trs = [dict(period=1, offset=0, end_exemptions=1, coeff=scalar()) for _ in range(prog_plain.n_transitions)]
        bnd = [(0, 0, 1, scalar()), (1, 0, 1, scalar())]
        bnd_rap = bnd + [(0, 0, scalar(), scalar(), True)]

        def old(prog=prog_plain, cs=consts[:n_consts], t_cols=cols[:n_cols], bnd=bnd, trs=trs):
            return X.constraint_evaluations_device(prog, cs, t_cols, LOG_TRACE, LOG_BLOWUP, bnd, trs, t_out=t_out, offset=3)

        def new(prog=prog_rap, cs=consts[:n_rap_consts], xs=xconsts[:n_xconsts], t_cols=cols[:n_main], bnd=bnd_rap, trs=trs):
            return X.rap_constraint_evaluations_device(prog, cs, xs, t_cols, aux, LOG_TRACE, LOG_BLOWUP, bnd, trs, t_out=t_out, offset=3)

        calls[f"{air} in F"], calls[f"{air} RAP"] = old, new
        t_old, t_new = timed(old), timed(new)
        print(f"RESULT {field} {air:<8} z a main column, challenges in F ({len(prog_plain)} ops) {fmt(t_old)}   z an auxiliary column, challenges in E "
              f"({len(prog_rap)} ops, one more boundary constraint, on z) {fmt(t_new)}   RAP / F = {ratio(t_new, t_old)}")
        if air == "rom":
            def same(prog=prog_plain, cs=consts, bnd=bnd, trs=trs):
                return X.rap_constraint_evaluations_device(prog, cs, [], cols, [], LOG_TRACE, LOG_BLOWUP, bnd, trs, t_out=t_out, offset=3)

            calls["rom all-F RAP entry"] = same
            t_same = timed(same)
            print(f"RESULT {field} all-F    the rom program with everything in F: existing entry {fmt(t_old)}   RAP entry {fmt(t_same)}   "
                  f"RAP entry / existing = {ratio(t_same, t_old)}")
    aux_product_ms = 0.0
    for label, call in calls.items():
        call()
        torch.cuda.synchronize()
        _lib.profile_begin()
        for _ in range(CALLS):
            call()
        torch.cuda.synchronize()
        for kname, (launches, ms) in sorted(_lib.profile_end().items()):
            print(f"KERNEL {field} {label:<20} {kname:<30} {launches / CALLS:g} per call  {ms / launches:8.4f} ms each")
            if label == "aux product":
                aux_product_ms += ms / CALLS
    # ---- PLONK round 2's grand product over as many rows, its three kernels alone (the call goes on to transform z)
    from lambda_elliptic_curves_amd import fft, plonk
    from tools import inputs
    el = lambda count, seed: inputs.rand_elems("fr381", count, seed)
    cir = plonk.Circuit(fft.FrField, n, inputs.offset_elem("fr381", 7), [el(n, 10 + j) for j in range(5)], [el(n, 20 + j) for j in range(3)],
                        [el(n, 30 + j) for j in range(3)])
    t_w = torch.from_numpy(el(3 * n, 1).view(np.int64)).cuda()
    beta, gamma, bl3 = el(1, 2)[0], el(1, 3)[0], el(3, 5)
    cir.round2_device(t_w, beta, gamma, bl3)
    torch.cuda.synchronize()
    _lib.profile_begin()
    for _ in range(CALLS):
        cir.round2_device(t_w, beta, gamma, bl3)
    torch.cuda.synchronize()
    plonk_ms = 0.0
    for kname, (launches, ms) in sorted(_lib.profile_end().items()):
        if kname.startswith("plonk_z_"):
            plonk_ms += ms / CALLS
            print(f"KERNEL {field} plonk round 2        {kname:<30} {launches / CALLS:g} per call  {ms / launches:8.4f} ms each")
    print(f"RESULT {field} aux product against PLONK round 2's grand product (BLS12-381 Fr), both over 2^{LOG_TRACE} rows, the three kernels of each: "
          f"{aux_product_ms:8.4f} ms, {aux_product_ms * 1e6 / n:.3f} ns per row, against {plonk_ms:8.4f} ms, {plonk_ms * 1e6 / n:.3f} ns per row   "
          f"aux product / plonk = {aux_product_ms / plonk_ms:.3f}")
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ext_rap.txt"))
    ap.add_argument("--step")
    args = ap.parse_args()
    if args.step:
        return step(args.step)
    me = os.path.abspath(__file__)
    lines = [f"# RAP over Fp2 / Fp4, trace 2^{LOG_TRACE}, blow-up {1 << LOG_BLOWUP}, N = 2^{LOG_TRACE + LOG_BLOWUP}: wall ms per call, median [min .. max] of {SAMPLES} samples of",
             f"# {CALLS} calls enqueued back to back after a warm-up, stream synchronised, every figure of a field in one process; the copy is torch's",
             "# device-to-device copy of half the bytes the call moves; the spread beside a ratio is the half range of both sides.",
             "# KERNEL lines: device time between events, from a run of its own in the same process."]
    rc, measured = 0, False
    for name, limit in STEPS:
        run = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, me, "--step", name], capture_output=True, text=True, cwd=ROOT)
        got = [ln[7:] for ln in run.stdout.splitlines() if ln.startswith(("RESULT ", "KERNEL "))]
        measured = measured or bool(got)
        lines += got
        print("\n".join(got), flush=True)
        if run.returncode:   # nothing more is started on the device after a step that failed or hung
            rc = run.returncode
            last = (run.stderr.strip().splitlines() or [""])[-1]
            lines.append(f"# step {name} stopped the run with exit status {rc}: {last[-300:]}")
            break
    if not measured:
        lines.append("not measured yet")
    print("\n".join(ln for ln in lines if ln.startswith("#") or ln == "not measured yet"), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return rc


if __name__ == "__main__":
    sys.exit(main())
