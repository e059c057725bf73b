#!/usr/bin/env python3
"""Goldilocks NTT on the device (csrc/goldilocks.hip) next to the BabyBear NTT on u64 words (csrc/ntt_bb.hip, layout
U64_R64): the same bytes through the same stages with a dearer product, timed in the same process.
  shape   goldilocks.ntt_device forward and inverse and fft.ntt_device at 1 x 2^20, 1 x 2^24, 4 x 2^22
  lde     goldilocks.lde_device and fft.lde_device with a coset offset at 4 x 2^22 -> 2^24
  kernels per-pass device times of one forward + one inverse (lw_hip_profile_begin / end) at 1 x 2^24 and 4 x 2^22, runs of
          their own
Every step is a process of its own under `timeout -k 10`; the first step that fails or hangs ends the run.
usage: goldilocks_timing.py [--out FILE]        (goldilocks_timing.py --step NAME runs one step)"""
import argparse
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STEPS = [("shape:1:20", 120), ("shape:1:24", 180), ("shape:4:22", 180), ("lde:4:22:24", 240), ("kernels:1:24", 180),
         ("kernels:4:22", 180)]
CALLS, SAMPLES = 10, 9
BB_P = 2013265921


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
    """u64 words below the BabyBear modulus: valid residues of either field"""
    import numpy as np
    import torch
    return torch.from_numpy(np.random.default_rng(seed).integers(0, BB_P, count, dtype=np.int64)).cuda()


def report(label, shape, g, b):
    # spread: half the range of the repeats of either side, relative to its median, added up
    ratio = g[0] / b[0]
    spread = ratio * ((g[2] - g[1]) / (2 * g[0]) + (b[2] - b[1]) / (2 * b[0]))
    print(f"RESULT {label:<10} {shape:<18} goldilocks {g[0]:8.4f} ms [{g[1]:8.4f} .. {g[2]:8.4f}]   babybear-u64 {b[0]:8.4f} ms [{b[1]:8.4f} .. {b[2]:8.4f}]"
          f"   goldilocks / babybear-u64 = {ratio:.3f} +- {spread:.3f}")


def step(name):
    import numpy as np
    import torch
    from lambda_elliptic_curves_amd import _lib, fft, goldilocks
    kind, *rest = name.split(":")
    bb = fft.Babybear31PrimeField
    if kind == "lde":
        batch, lin, lout = (int(v) for v in rest)
        t_in = words(batch << lin, 3)
        t_out = torch.empty(batch << lout, dtype=torch.int64, device="cuda")
        off = np.array([7], np.uint64)
        g = timed(lambda: goldilocks.lde_device(t_in, lin, t_out, lout, batch=batch, offset=7))
        b = timed(lambda: fft.lde_device(bb, t_in, lin, t_out, lout, batch=batch, offset=off))
        report("coset lde", f"{batch} x 2^{lin} -> 2^{lout}", g, b)
        return 0
    batch, L = (int(v) for v in rest)
    t_in = words(batch << L, 1)
    t_out = torch.empty_like(t_in)
    fwd = lambda: goldilocks.ntt_device(t_in, t_out, L, batch=batch)
    inv = lambda: goldilocks.ntt_device(t_in, t_out, L, inverse=True, batch=batch)
    ref = lambda: fft.ntt_device(bb, t_in, t_out, L, batch=batch)
    if kind == "kernels":
        fwd(), inv(), ref()   # tables, scratch
        torch.cuda.synchronize()
        for label, fn in (("goldilocks forward", fwd), ("goldilocks inverse", inv), ("babybear-u64 forward", ref)):
            _lib.profile_begin()
            for _ in range(CALLS):
                fn()
            torch.cuda.synchronize()
            for kname, (launches, ms) in sorted(_lib.profile_end().items()):
                print(f"KERNEL {batch} x 2^{L}  {label:<22} {kname:<24} {launches // CALLS} per call  {ms / launches:8.4f} ms each")
        return 0
    f, i, b = timed(fwd), timed(inv), timed(ref)
    report("forward", f"{batch} x 2^{L}", f, b)
    report("inverse", f"{batch} x 2^{L}", i, b)
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "goldilocks_ntt.txt"))
    ap.add_argument("--step")
    args = ap.parse_args()
    if args.step:
        return step(args.step)
    me = os.path.abspath(__file__)
    lines = [f"# Goldilocks NTT against the BabyBear NTT on u64 words (U64_R64, forward): wall ms per call, median [min .. max] of {SAMPLES} samples of",
             f"# {CALLS} calls enqueued back to back after a warm-up, stream synchronised; the spread beside a ratio is the half range of both sides"]
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
