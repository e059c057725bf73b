#!/usr/bin/env python3
"""The fused constraint pass of circle STARK round 2 over Mersenne31 with QM31 (csrc/circle_round2.cuh) next to the same pass
over BabyBear with Fp4 (csrc/ext_round2.cuh) and next to a device copy of the bytes the call must move, all timed in the
same process: trace 2^20, blow-up 4, the two-column Fibonacci and the read-only-memory programs of tools/ext_round2_timing.py,
two boundary constraints on one step.
  call     wall time of mersenne31_ext.constraint_evaluations_device: the point table, the cycle tables, the fused kernel,
           one boundary launch
  fp4      wall time of babybear_ext.constraint_evaluations_device at the same shape (both fields have 4-byte words and four
           planes, so both calls move the same bytes)
  copy     torch's device-to-device copy of the columns read once plus the four planes written once
  kernels  device time of every kernel of the call (lw_hip_profile_begin / end), a run of its own, and its share of their sum
Nothing here has an earlier measurement to be compared with and no threshold is set: the ratios to Fp4 and to the copy are the
figures.  Every step is a process of its own under `timeout -k 10`; the first step that fails or hangs ends the run.
usage: circle_round2_timing.py [--out FILE]        (circle_round2_timing.py --step NAME runs one step)"""
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
M31_P, BB_P = (1 << 31) - 1, 2013265921
AIRS = {"fib2": ("fibonacci, 2 columns", 2, 0), "rom": ("read-only memory, permutation", 5, 3)}
STEPS = [(air, 240) for air in AIRS]


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


def programs(stark):
    one, z, alpha = stark.const(0), stark.const(1), stark.const(2)
    step = stark.cell(2, 1) - stark.cell(2) - one
    return {"fib2": [stark.cell(0, 1) - stark.cell(1), stark.cell(1, 1) - stark.cell(0) - stark.cell(1)],
            "rom": [(stark.cell(2, 1) - stark.cell(2)) * step, (stark.cell(3, 1) - stark.cell(3)) * step,
                    (z - (stark.cell(2, 1) + alpha * stark.cell(3, 1))) * stark.cell(4, 1) - (z - (stark.cell(0, 1) + alpha * stark.cell(1, 1))) * stark.cell(4)]}


def step(air):
    import numpy as np
    import torch
    from lambda_elliptic_curves_amd import _lib, babybear_ext, mersenne31_ext, stark
    label, n_cols, n_consts = AIRS[air]
    N = 1 << (LOG_TRACE + LOG_BLOWUP)
    program = stark.compile_transitions(programs(stark)[air])
    calls = {}
    for name, X, p in (("m31q", mersenne31_ext, M31_P), ("fp4", babybear_ext, BB_P)):
        rng = np.random.default_rng(1)
        cols = [torch.from_numpy(rng.integers(0, p, N, dtype=np.uint32).view(np.int32)).cuda() for _ in range(n_cols)]
        scalar = lambda: tuple(int(v) for v in rng.integers(1, p, 4, dtype=np.uint32))
        consts = [int(v) for v in rng.integers(1, p, n_consts, dtype=np.uint32)]
        transitions = [dict(period=1, offset=0, end_exemptions=1, coeff=scalar()) for _ in range(program.n_transitions)]
        boundary = [(0, 0, 1, scalar()), (1, 0, 1, scalar())]
        t_out = torch.empty(4 * N, dtype=torch.int32, device="cuda")
        extra = {} if name == "m31q" else {"offset": 3}
        calls[name] = (lambda X=X, consts=consts, cols=cols, boundary=boundary, transitions=transitions, t_out=t_out, extra=extra:
                       X.constraint_evaluations_device(program, consts, cols, LOG_TRACE, LOG_BLOWUP, boundary, transitions, t_out=t_out, **extra))
    moved = (n_cols + 4) * N * 4                               # columns read once, four planes written once
    src = torch.zeros(moved // 2, dtype=torch.uint8, device="cuda")
    dst = torch.empty_like(src)
    t, f, c = timed(calls["m31q"]), timed(calls["fp4"]), timed(lambda: dst.copy_(src))
    print(f"RESULT {label:<30} ops {len(program):3d} tmps {program.n_tmps}  call {fmt(t)}   fp4 {fmt(f)}   copy of {moved / 2**20:6.1f} MiB moved {fmt(c)}   "
          f"call / fp4 = {ratio(t, f)}   call / copy = {ratio(t, c)}")
    for name in ("m31q", "fp4"):
        calls[name]()
        torch.cuda.synchronize()
        _lib.profile_begin()
        for _ in range(CALLS):
            calls[name]()
        torch.cuda.synchronize()
        prof = _lib.profile_end()
        total = sum(ms for _, ms in prof.values())
        for kname, (launches, ms) in sorted(prof.items()):
            print(f"KERNEL {label:<30} {kname:<26} {launches / CALLS:g} per call  {ms / launches:8.4f} ms each   share {ms / total:5.1%}   / copy = {ms / launches / c[0]:.2f}")
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "circle_round2.txt"))
    ap.add_argument("--step")
    args = ap.parse_args()
    if args.step:
        return step(args.step)
    me = os.path.abspath(__file__)
    lines = [f"# Circle round 2 over QM31, trace 2^{LOG_TRACE}, blow-up {1 << LOG_BLOWUP}, N = 2^{LOG_TRACE + LOG_BLOWUP}, 2 boundary constraints on one step: wall ms per call,",
             f"# median [min .. max] of {SAMPLES} samples of {CALLS} calls enqueued back to back after a warm-up, stream synchronised; fp4 is",
             "# babybear_ext.constraint_evaluations_device at the same shape in the same process; the copy is torch's device-to-device copy of half the",
             "# bytes the call moves (read once, written once); the spread beside a ratio is the half range of both sides.  KERNEL lines: device time",
             "# between events and the kernel's share of the call's kernels, from a run of its own in the same process (m31q_* then bb4_*)."]
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
