#!/usr/bin/env python3
"""Circle FFT over Mersenne31 on the device (csrc/circle.hip) next to the BabyBear NTT (csrc/ntt_bb.hip, layout U32_R32): the
same bytes through the same number of passes with a dearer product, timed in the same process.
  shape   circle.evaluate_cfft_device, circle.interpolate_cfft_device and fft.ntt_device at 1 x 2^20, 1 x 2^24, 4 x 2^24
  lde     circle.lde_device and fft.lde_device at 4 x 2^22 -> 2^24
  kernels per-kernel device times of one evaluate + one interpolate at 4 x 2^24 (lw_hip_profile_begin / end), a run of its own
Every step is a process of its own under `timeout -k 10`, chained with &&: a step that fails or hangs ends the run.
usage: circle_timing.py [--out FILE]        (circle_timing.py --step NAME runs one step)"""
import argparse
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STEPS = [("shape:1:20", 120), ("shape:1:24", 180), ("shape:4:24", 240), ("lde:4:22:24", 240), ("kernels:4:24", 240)]
CALLS, SAMPLES = 10, 9


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


def words(count, seed):
    import numpy as np
    import torch
    w = np.random.default_rng(seed).integers(0, 2013265921, count, dtype=np.int64).astype(np.int32)
    return torch.from_numpy(w).cuda()


def report(label, shape, c, b):
    # spread: half the range of the repeats of either side, relative to its median, added up
    ratio = c[0] / b[0]
    spread = ratio * ((c[2] - c[1]) / (2 * c[0]) + (b[2] - b[1]) / (2 * b[0]))
    print(f"RESULT {label:<12} {shape:<16} circle {c[0]:8.4f} ms [{c[1]:8.4f} .. {c[2]:8.4f}]   babybear {b[0]:8.4f} ms [{b[1]:8.4f} .. {b[2]:8.4f}]"
          f"   circle / babybear = {ratio:.3f} +- {spread:.3f}")


def step(name):
    import torch
    from lambda_elliptic_curves_amd import _lib, circle, fft
    kind, *rest = name.split(":")
    bb = fft.Babybear31PrimeFieldU32
    if kind == "lde":
        batch, lin, lout = (int(v) for v in rest)
        t_in = words(batch << lin, 3)
        t_out = torch.empty(batch << lout, dtype=torch.int32, device="cuda")
        c = timed(lambda: circle.lde_device(t_in, lin, t_out, lout, batch=batch))
        b = timed(lambda: fft.lde_device(bb, t_in, lin, t_out, lout, batch=batch))
        print("# circle: evaluations -> evaluations (interpolate, then evaluate); babybear: coefficients -> evaluations (evaluate only)")
        report("lde", f"{batch} x 2^{lin} -> 2^{lout}", c, b)
        return 0
    batch, L = (int(v) for v in rest)
    t_in = words(batch << L, 1)
    t_out = torch.empty_like(t_in)
    if kind == "kernels":
        circle.evaluate_cfft_device(t_in, t_out, L, batch=batch)   # tables, scratch
        circle.interpolate_cfft_device(t_in, t_out, L, batch=batch)
        fft.ntt_device(bb, t_in, t_out, L, batch=batch)
        torch.cuda.synchronize()
        _lib.profile_begin()
        for _ in range(CALLS):
            circle.evaluate_cfft_device(t_in, t_out, L, batch=batch)
            circle.interpolate_cfft_device(t_in, t_out, L, batch=batch)
            fft.ntt_device(bb, t_in, t_out, L, batch=batch)
        torch.cuda.synchronize()
        for kname, (launches, ms) in sorted(_lib.profile_end().items()):
            print(f"KERNEL {batch} x 2^{L}  {kname:<32} {launches:4d} launches  {ms / launches:8.4f} ms each")
        return 0
    ev = timed(lambda: circle.evaluate_cfft_device(t_in, t_out, L, batch=batch))
    it = timed(lambda: circle.interpolate_cfft_device(t_in, t_out, L, batch=batch))
    b = timed(lambda: fft.ntt_device(bb, t_in, t_out, L, batch=batch))
    report("evaluate", f"{batch} x 2^{L}", ev, b)
    report("interpolate", f"{batch} x 2^{L}", it, b)
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "circle_fft.txt"))
    ap.add_argument("--step")
    args = ap.parse_args()
    if args.step:
        return step(args.step)
    me = os.path.abspath(__file__)
    chain = " && ".join(f"timeout -k 10 {limit} {sys.executable} {me} --step {name}" for name, limit in STEPS)
    run = subprocess.run(chain, shell=True, capture_output=True, text=True, cwd=ROOT)
    lines = [f"# Circle FFT over Mersenne31 against the BabyBear NTT (U32_R32, forward): wall ms per call, median [min .. max] of {SAMPLES} samples of",
             f"# {CALLS} calls enqueued back to back after a warm-up, stream synchronised; the spread beside a ratio is the half range of both sides"]
    lines += [ln[7:] if ln.startswith(("RESULT ", "KERNEL ")) else ln for ln in run.stdout.splitlines() if ln.startswith(("RESULT", "KERNEL", "#"))]
    if not any(ln.startswith("RESULT") for ln in run.stdout.splitlines()):
        lines.append("not measured yet")
    if run.returncode:
        lines.append(f"# the chain stopped with exit status {run.returncode}: {run.stderr[-400:].strip()}")
    print("\n".join(lines), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return run.returncode


if __name__ == "__main__":
    sys.exit(main())
