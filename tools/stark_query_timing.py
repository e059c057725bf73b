#!/usr/bin/env python3
"""STARK round 4 tail on the device (csrc/stark_query.hip):
  1. candidates per second of the grinding search kernel for the windows of grinding factors 20, 24 and 28, specialised
     permutation against the unmodified keccak_f1600 in the same loop (tools/stark_grind_bench, built by build());
  2. wall time of whole stark.grinding_nonce calls on a fixed seed (inner hash, windows, read-backs), 9 calls after a warm-up;
  3. stark.fri_query_phase_device over the layers of a 2^20-coefficient FRI commit phase at 30 queries, next to the bytes a
     host-side query phase would have had to copy back (every layer's evaluation and nodes).
usage: stark_query_timing.py [--out FILE]"""
import argparse
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from lambda_elliptic_curves_amd import fft, merkle, stark  # noqa: E402
from tools import inputs  # noqa: E402

SEED = bytes([37, 68, 26, 150, 139, 142, 66, 175, 33, 47, 199, 160, 9, 109, 79, 234, 135, 254, 39, 11, 225, 219, 206, 108, 224,
              165, 25, 72, 189, 96, 218, 95])   # provers/stark/src/grinding.rs:117-120


def timed(fn, reps=9):
    fn()
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        out.append((time.perf_counter() - t0) * 1e3)
    return r, statistics.median(out), min(out), max(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stark_grinding.txt"))
    args = ap.parse_args()
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    emit(f"# {torch.cuda.get_device_name(0)}")
    emit("# 1. search kernel alone, one window per launch, no candidate passes: median [min .. max] of 9 launches after a warm-up")
    bench = subprocess.run([os.path.join(ROOT, "tools", "stark_grind_bench"), "20", "24", "28"], capture_output=True, text=True, timeout=300)
    for ln in (bench.stdout + bench.stderr).splitlines():
        emit(ln)
    if bench.returncode:
        emit(f"# stark_grind_bench exited with {bench.returncode}")
        return 1
    emit("# 2. whole calls, stark.grinding_nonce(seed B of grinding.rs, factor, first = 0): wall ms, median [min .. max] of 9 after a warm-up")
    for g in (20, 24, 28):
        nonce, med, lo, hi = timed(lambda: stark.grinding_nonce(SEED, g))
        emit(f"factor {g}: nonce {nonce:#x}, window 2^{stark.grinding_window(g).bit_length() - 1}, {med:8.3f} ms [{lo:8.3f} .. {hi:8.3f}], "
             f"{(nonce + 1) / med / 1e6:6.3f} G candidates/s up to the hit")
    emit("# 3. fri_query_phase_device, Stark252, 2^20 coefficients on a 2^21 domain, 20 layers, 30 queries")
    F, n, domain = fft.Stark252PrimeField, 1 << 20, 1 << 21
    a = inputs.rand_elems("stark252", n, 5)
    zetas = iter(inputs.rand_elems("stark252", 32, 6))
    offs = inputs.rand_elems("stark252", 32, 7)
    _, layers = merkle.fri_commit_phase_device(F, 21, torch.from_numpy(a.view(np.int64)).cuda(), n, lambda: next(zetas), lambda root: None,
                                               lambda k: offs[k], domain)
    iotas = [int(x) for x in np.random.default_rng(8).integers(0, domain // 2, 30)]
    res, med, lo, hi = timed(lambda: stark.fri_query_phase_device(F, layers, iotas))
    out_b = len(iotas) * (32 * len(layers) + sum(p.nbytes for p in res[0][1]))
    back_b = sum(d * 32 + (d - 1) * 32 for _, _, _, d in layers)
    emit(f"{len(layers)} layers, {len(iotas)} queries: {med:8.3f} ms [{lo:8.3f} .. {hi:8.3f}] per call, {out_b} bytes of openings returned; "
         f"a host-side query phase copies back {back_b} bytes ({back_b / 2**20:.1f} MiB) of evaluations and nodes first")
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
