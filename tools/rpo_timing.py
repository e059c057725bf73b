#!/usr/bin/env python3
"""Rescue Prime Optimized on the device (csrc/rpo.hip): permutations per second next to the ceiling the arithmetic sets.
  gl_mul     the Goldilocks product rate of tools/microbench (built by build()); one permutation is 7 x m x 76 products,
             6384 at the 128-bit level and 8512 at the 160-bit level, so rate / 6384 (8512) is the ceiling in
             permutations/s.  The MDS layers are NOT in that count: their cost shows as distance from the ceiling.
  permute    rpo.permute_device at 2^16 and 2^20 states, both levels; one state through permute_device and through permute (the call itself)
  commit     rpo.commit_columns_device for 8 x 2^20 and 1 x 2^20, both levels
Every step is a process of its own under `timeout -k 10`, chained with &&: a step that fails or hangs ends the run.
usage: rpo_timing.py [--out FILE]        (rpo_timing.py --step NAME runs one step)"""
import argparse
import os
import re
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PRODUCTS = {0: 7 * 12 * 76, 1: 7 * 16 * 76}   # level -> gl_mul per permutation: x^7 is 4 products, x^(1/7) 72
NAMES = {0: "128", 1: "160"}
# a trailing ":host" times the host form (staged, complete on return); at 2^0 a line is the cost of the call itself
STEPS = [("gl_mul", 240), ("permute:0:0", 120), ("permute:0:0:host", 120)]
STEPS += [(f"permute:{lv}:{k}", 120) for lv in (0, 1) for k in (16, 20)]
STEPS += [(f"commit:{lv}:{c}:20", 180) for lv in (0, 1) for c in (8, 1)]


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
    if name == "gl_mul":
        r = subprocess.run([os.path.join(ROOT, "tools", "microbench")], capture_output=True, text=True)
        m = re.search(r"RATE gl_mul Goldilocks\s+([0-9.]+) Gmul/s", r.stdout)
        if r.returncode or not m:
            print(r.stdout[-2000:] + r.stderr[-2000:])
            return 1
        print(f"GL_MUL {m.group(1)} Gmul/s (tools/microbench, gl_mul Goldilocks, all CUs)")
        return 0
    import numpy as np
    import torch
    from lambda_elliptic_curves_amd import rpo
    rng = np.random.default_rng(43)
    dev = lambda a: torch.from_numpy(a.view(np.int64)).cuda()
    kind, lv, *rest = name.split(":")
    level = int(lv)
    if kind == "permute":
        n = 1 << int(rest[0])
        host = rest[1:] == ["host"]
        t = rng.integers(0, 1 << 64, n * rpo.state_width(level), dtype=np.uint64)
        t = t if host else dev(t)
        med, lo, hi = timed((lambda: rpo.permute(level, t)) if host else (lambda: rpo.permute_device(level, t, n)), reps=201 if n == 1 else 9)
        print(f"RESULT {level} RPO-{NAMES[level]} permute{'' if host else '_device'} 2^{rest[0]}: {n} permutations, {med:9.3f} ms [{lo:9.3f} .. {hi:9.3f}] PERMS {n / med * 1e3:.6e}")
        return 0
    n_cols, log2n = int(rest[0]), int(rest[1])
    n = 1 << log2n
    t_cols = dev(rng.integers(0, 1 << 64, n_cols * n, dtype=np.uint64))
    t_nodes = torch.empty((2 * n - 1, rpo.digest_len(level)), dtype=torch.int64, device="cuda")
    perms = n * -(-n_cols // rpo.rate(level)) + n - 1   # leaves: one permutation per block of the row; one per node
    med, lo, hi = timed(lambda: rpo.commit_columns_device(level, t_cols, n_cols, log2n, t_nodes, True, return_root=False), reps=5)
    print(f"RESULT {level} RPO-{NAMES[level]} commit_columns_device {n_cols} x 2^{log2n}: {perms} permutations, {med:9.3f} ms [{lo:9.3f} .. {hi:9.3f}] PERMS {perms / med * 1e3:.6e}")
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rpo.txt"))
    ap.add_argument("--step")
    args = ap.parse_args()
    if args.step:
        return step(args.step)
    me = os.path.abspath(__file__)
    chain = " && ".join(f"timeout -k 10 {limit} {sys.executable} {me} --step {name}" for name, limit in STEPS)
    run = subprocess.run(chain, shell=True, capture_output=True, text=True, cwd=ROOT)
    lines = ["# Rescue Prime Optimized over Goldilocks: wall ms per call, median [min .. max] after a warm-up (9 calls; 201 at 2^0; trees 5), stream synchronised"]
    rate_mul = None
    for ln in run.stdout.splitlines():
        if ln.startswith("GL_MUL"):
            rate_mul = float(ln.split()[1]) * 1e9
            lines.append(f"{ln}; ceiling = rate / {PRODUCTS[0]} = {rate_mul / PRODUCTS[0]:.4e} permutations/s (RPO-128), "
                         f"rate / {PRODUCTS[1]} = {rate_mul / PRODUCTS[1]:.4e} (RPO-160)")
        elif ln.startswith("RESULT"):
            level = int(ln.split()[1])
            rate = float(ln.rsplit("PERMS", 1)[1])
            text = ln.split(" ", 2)[2].rsplit("PERMS", 1)[0]
            lines.append(f"{text}{rate:.4e} permutations/s"
                         + (f" = {rate / (rate_mul / PRODUCTS[level]):.3f} of the {PRODUCTS[level]}-product ceiling {rate_mul / PRODUCTS[level]:.4e}" if rate_mul else ""))
    if run.returncode:
        lines.append(f"# the chain stopped with exit status {run.returncode}: {run.stderr[-400:].strip()}")
    print("\n".join(lines), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return run.returncode


if __name__ == "__main__":
    sys.exit(main())
