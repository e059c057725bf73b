#!/usr/bin/env python3
"""Monolith over Mersenne31 on the device (csrc/monolith.hip): permutations per second next to the ceiling the arithmetic
sets and next to a copy of the same bytes.
  mac        the v_mad_u64_u32 rate of tools/microbench (built by build()): acc += (u64) a * b, the multiply-add of Concrete.
             A width-16 permutation with R = 5 runs 7 Concrete layers of 256 multiply-adds, so rate / 1792 is the ceiling
             in permutations/s (width 24: 7 x 576 = 4032).  Bars, Bricks and the reductions are NOT in that count: their
             cost shows as distance from the ceiling.
  permute    monolith.permute_device at 2^20 and 2^24 states for (16, 5) and 2^20 for (24, 5), and a device-to-device
             copy of the same bytes; one state of (16, 5) through permute_device and through permute (the call itself)
  commit     monolith.commit_columns_device for 8 x 2^20 and 1 x 2^24 at R = 5, with the time of each of the three tree
             kernels (the shared schedule of hash_tree.cuh: one pair launch per wide level, the top kernel from 2^9 nodes)
Every step is a process of its own under `timeout -k 10`, chained with &&: a step that fails or hangs ends the run.
usage: monolith_timing.py [--out FILE]        (monolith_timing.py --step NAME runs one step)"""
import argparse
import os
import re
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ROUNDS = 5
MACS = {16: 7 * 256, 24: 7 * 576}   # width -> multiply-adds of the R + 2 = 7 Concrete layers
# a trailing ":host" times the host form (staged, complete on return); at 2^0 a line is the cost of the call itself
STEPS = [("mac", 240), ("permute:16:0", 120), ("permute:16:0:host", 120), ("permute:16:20", 120), ("permute:16:24", 180), ("permute:24:20", 120), ("commit:8:20", 180), ("commit:1:24", 180)]


def timed(fn, reps=9):
    import torch
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(out), min(out), max(out)


def step(name):
    if name == "mac":
        r = subprocess.run([os.path.join(ROOT, "tools", "microbench")], capture_output=True, text=True)
        m = re.search(r"RATE v_mad_u64_u32\s+([0-9.]+) Gop/s", r.stdout)
        if r.returncode or not m:
            print(r.stdout[-2000:] + r.stderr[-2000:])
            return 1
        print(f"MAC {m.group(1)} Gmac/s (tools/microbench, v_mad_u64_u32, 8 independent chains a work-item, all CUs)")
        return 0
    import numpy as np
    import torch
    from lambda_elliptic_curves_amd import _lib, monolith
    rng = np.random.default_rng(47)
    dev = lambda a: torch.from_numpy(a.view(np.int32)).cuda()
    kind, a, b, *host = name.split(":")
    if kind == "permute":
        width, n = int(a), 1 << int(b)
        t = rng.integers(0, 1 << 32, n * width, dtype=np.uint32)
        if host:
            med, lo, hi = timed(lambda: monolith.permute(width, ROUNDS, t), reps=201)
            print(f"RESULT {width} Monolith-{width} R={ROUNDS} permute 2^{b}: {n} permutations, {med:9.3f} ms [{lo:9.3f} .. {hi:9.3f}] PERMS {n / med * 1e3:.6e}")
            return 0
        t = dev(t)
        t_out = torch.empty_like(t)
        med, lo, hi = timed(lambda: monolith.permute_device(width, ROUNDS, t, n, t_out), reps=201 if n == 1 else 9)
        c_med, c_lo, c_hi = timed(lambda: t_out.copy_(t))
        print(f"RESULT {width} Monolith-{width} R={ROUNDS} permute_device 2^{b}: {n} permutations, {med:9.3f} ms [{lo:9.3f} .. {hi:9.3f}]; "
              f"copy of the same {4 * n * width} bytes {c_med:9.3f} ms [{c_lo:9.3f} .. {c_hi:9.3f}], ratio {med / c_med:.2f} PERMS {n / med * 1e3:.6e}")
        return 0
    n_cols, log2n = int(a), int(b)
    n = 1 << log2n
    t_cols = dev(rng.integers(0, 1 << 32, n_cols * n, dtype=np.uint32))
    t_nodes = torch.empty((2 * n - 1, 8), dtype=torch.int32, device="cuda")
    perms = n * -(-n_cols // monolith.RATE) + n - 1   # leaves: one permutation per chunk of the row; one per node
    run = lambda: monolith.commit_columns_device(ROUNDS, t_cols, n_cols, log2n, t_nodes, True, return_root=False)
    med, lo, hi = timed(run, reps=5)
    _lib.profile_begin()
    run()
    torch.cuda.synchronize()
    prof = _lib.profile_end()
    parts = ", ".join(f"{k} {v[0]} x = {v[1]:.3f} ms" for k, v in sorted(prof.items()))
    print(f"RESULT 16 Monolith-16 R={ROUNDS} commit_columns_device {n_cols} x 2^{log2n}: {perms} permutations, {med:9.3f} ms [{lo:9.3f} .. {hi:9.3f}]"
          f" ({parts}) PERMS {perms / med * 1e3:.6e}")
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "monolith.txt"))
    ap.add_argument("--step")
    args = ap.parse_args()
    if args.step:
        return step(args.step)
    me = os.path.abspath(__file__)
    chain = " && ".join(f"timeout -k 10 {limit} {sys.executable} {me} --step {name}" for name, limit in STEPS)
    run = subprocess.run(chain, shell=True, capture_output=True, text=True, cwd=ROOT)
    lines = ["# Monolith over Mersenne31: wall ms per call, median [min .. max] after a warm-up (9 calls; 201 at 2^0; trees 5), stream synchronised"]
    rate_mac = None
    for ln in run.stdout.splitlines():
        if ln.startswith("MAC"):
            rate_mac = float(ln.split()[1]) * 1e9
            lines.append(f"{ln}; ceiling = rate / {MACS[16]} = {rate_mac / MACS[16]:.4e} permutations/s (width 16), "
                         f"rate / {MACS[24]} = {rate_mac / MACS[24]:.4e} (width 24)")
        elif ln.startswith("RESULT"):
            width = int(ln.split()[1])
            rate = float(ln.rsplit("PERMS", 1)[1])
            text = ln.split(" ", 2)[2].rsplit("PERMS", 1)[0]
            lines.append(f"{text}{rate:.4e} permutations/s"
                         + (f" = {rate / (rate_mac / MACS[width]):.3f} of the {MACS[width]}-MAC ceiling {rate_mac / MACS[width]:.4e}" if rate_mac else ""))
    if run.returncode:
        lines.append(f"# the chain stopped with exit status {run.returncode}: {run.stderr[-400:].strip()}")
    print("\n".join(lines), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return run.returncode


if __name__ == "__main__":
    sys.exit(main())
