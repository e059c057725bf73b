#!/usr/bin/env python3
"""The fused constraint pass of round 2 over Goldilocks with Fp2 and BabyBear with Fp4 (csrc/ext_round2.cuh) next to a device
copy of the bytes the call must move, timed in the same process: trace 2^20, blow-up 4, the two-column Fibonacci and the
read-only-memory programs (the shapes of profiles/air_program.txt), both fields.
  call     wall time of constraint_evaluations_device: the cycle tables, the fused kernel, one boundary launch
  copy     torch's device-to-device copy of the columns read once plus the D output planes written once
  kernels  device time of every kernel of the call (lw_hip_profile_begin / end), a run of its own
  avoided  the bytes a round trip of the T_c rows (n_transitions x N words written and read) would have added
Nothing here has an earlier measurement to be compared with: the ratio to the copy is the figure.
Every step is a process of its own under `timeout -k 10`; the first step that fails or hangs ends the run.
usage: ext_round2_timing.py [--out FILE]        (ext_round2_timing.py --step NAME runs one step)"""
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
AIRS = {"fib2": ("fibonacci, 2 columns", 2, 0), "rom": ("read-only memory, permutation", 5, 3)}
STEPS = [(f"{field}:{air}", 240) for field in ("gl2", "bb4") for air in AIRS]


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


def programs(stark):
    one, z, alpha = stark.const(0), stark.const(1), stark.const(2)
    step = stark.cell(2, 1) - stark.cell(2) - one
    return {"fib2": [stark.cell(0, 1) - stark.cell(1), stark.cell(1, 1) - stark.cell(0) - stark.cell(1)],
            "rom": [(stark.cell(2, 1) - stark.cell(2)) * step, (stark.cell(3, 1) - stark.cell(3)) * step,
                    (z - (stark.cell(2, 1) + alpha * stark.cell(3, 1))) * stark.cell(4, 1) - (z - (stark.cell(0, 1) + alpha * stark.cell(1, 1))) * stark.cell(4)]}


def step(name):
    import numpy as np
    import torch
    from lambda_elliptic_curves_amd import _lib, babybear_ext, goldilocks_ext, stark
    field, air = name.split(":")
    label, n_cols, n_consts = AIRS[air]
    X, p, width, word_bytes, np_word, signed = ((goldilocks_ext, GL_P, 2, 8, np.uint64, np.int64) if field == "gl2" else
                                                (babybear_ext, BB_P, 4, 4, np.uint32, np.int32))
    N = 1 << (LOG_TRACE + LOG_BLOWUP)
    rng = np.random.default_rng(1)
    cols = [torch.from_numpy(rng.integers(0, p, N, dtype=np_word).view(signed)).cuda() for _ in range(n_cols)]
    program = stark.compile_transitions(programs(stark)[air])
    scalar = lambda: tuple(int(v) for v in rng.integers(1, p, width, dtype=np_word))
    consts = [int(v) for v in rng.integers(1, p, n_consts, dtype=np_word)]
    transitions = [dict(period=1, offset=0, end_exemptions=1, coeff=scalar()) for _ in range(program.n_transitions)]
    boundary = [(0, 0, 1, scalar()), (1, 0, 1, scalar())]
    t_out = torch.empty(width * N, dtype=cols[0].dtype, device="cuda")
    call = lambda: X.constraint_evaluations_device(program, consts, cols, LOG_TRACE, LOG_BLOWUP, boundary, transitions, t_out=t_out, offset=3)
    moved = (n_cols + width) * N * word_bytes                  # columns read once, D planes written once
    src = torch.zeros(moved // 2, dtype=torch.uint8, device="cuda")
    dst = torch.empty_like(src)
    t, c = timed(call), timed(lambda: dst.copy_(src))
    ratio = t[0] / c[0]
    spread = ratio * ((t[2] - t[1]) / (2 * t[0]) + (c[2] - c[1]) / (2 * c[0]))
    avoided = 2 * program.n_transitions * N * word_bytes
    print(f"RESULT {field} {label:<30} ops {len(program):3d} tmps {program.n_tmps}  call {fmt(t)}   copy of {moved / 2**20:6.1f} MiB moved {fmt(c)}   "
          f"call / copy = {ratio:.2f} +- {spread:.2f}   a T_c round trip would add {avoided / 2**20:6.1f} MiB ({avoided / moved:.2f} x the bytes moved)")
    call()
    torch.cuda.synchronize()
    _lib.profile_begin()
    for _ in range(CALLS):
        call()
    torch.cuda.synchronize()
    for kname, (launches, ms) in sorted(_lib.profile_end().items()):
        print(f"KERNEL {field} {label:<30} {kname:<26} {launches / CALLS:g} per call  {ms / launches:8.4f} ms each   / copy = {ms / launches / c[0]:.2f}")
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ext_round2.txt"))
    ap.add_argument("--step")
    args = ap.parse_args()
    if args.step:
        return step(args.step)
    me = os.path.abspath(__file__)
    lines = [f"# Round 2 over Fp2 / Fp4, trace 2^{LOG_TRACE}, blow-up {1 << LOG_BLOWUP}, N = 2^{LOG_TRACE + LOG_BLOWUP}, 2 boundary constraints on one step: wall ms per call,",
             f"# median [min .. max] of {SAMPLES} samples of {CALLS} calls enqueued back to back after a warm-up, stream synchronised; the copy is torch's",
             "# device-to-device copy of half the bytes the call moves (read once, written once); the spread beside a ratio is the half range of",
             "# both sides.  KERNEL lines: device time between events, from a run of its own in the same process."]
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
