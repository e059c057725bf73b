#!/usr/bin/env python3
"""Starknet Poseidon on the device (csrc/poseidon.hip): permutations per second next to the ceiling the arithmetic sets.
  fe_mul     the Stark252 Montgomery product rate of tools/microbench (built by build()); one permutation is 214 products,
             so rate / 214 is the ceiling in permutations/s
  permute    poseidon.permute_device at 2^20 and 2^24 states; one state through permute_device and through permute (the call itself)
  commit     poseidon.commit_columns_device for 1 x 2^20 and 1 x 2^24 (TreePoseidon) and 4 x 2^22 (BatchPoseidonTree)
Every step is a process of its own under `timeout -k 10`, chained with &&: a step that fails or hangs ends the run.
usage: poseidon_timing.py [--out FILE]        (poseidon_timing.py --step NAME runs one step)"""
import argparse
import os
import re
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PRODUCTS = 214   # 8 full rounds x 3 S-boxes x 2 + 83 partial rounds x 2
# single-thread CPU figure, DERIVED: bench.py's cpu_baseline leg ran one Stark252 evaluate_fft of 2^24 elements at 2.04 M
# elements/s (BENCH_r03.json), 12 products per element -> at most 41 ns per product -> 8.7 us per permutation
CPU_NS_PER_PRODUCT = 1e9 / (2041730.9 * 12)
# a trailing ":host" times the host form (staged, complete on return); at 2^0 a line is the cost of the call itself
STEPS = [("fe_mul", 240), ("permute:0", 120), ("permute:0:host", 120), ("permute:20", 120), ("permute:24", 180), ("commit:1:20:single", 120), ("commit:1:24:single", 240),
         ("commit:4:22:many", 240)]


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
    if name == "fe_mul":
        r = subprocess.run([os.path.join(ROOT, "tools", "microbench")], capture_output=True, text=True)
        m = re.search(r"RATE fe_mul Stark252\s+([0-9.]+) Gmul/s", r.stdout)
        if r.returncode or not m:
            print(r.stdout[-2000:] + r.stderr[-2000:])
            return 1
        print(f"FE_MUL {m.group(1)} Gmul/s (tools/microbench, fe_mul Stark252, all CUs)")
        return 0
    import numpy as np
    import torch
    from lambda_elliptic_curves_amd import poseidon
    from tools import inputs
    dev = lambda a: torch.from_numpy(a.view(np.int64)).cuda()
    kind, *rest = name.split(":")
    if kind == "permute":
        n = 1 << int(rest[0])
        host = rest[1:] == ["host"]
        t = inputs.rand_elems("stark252", 3 * n, 41) if host else dev(inputs.rand_elems("stark252", 3 * n, 41))
        med, lo, hi = timed((lambda: poseidon.permute(t)) if host else (lambda: poseidon.permute_device(t, n)), reps=201 if n == 1 else 9)
        print(f"RESULT permute{'' if host else '_device'} 2^{rest[0]}: {n} permutations, {med:9.3f} ms [{lo:9.3f} .. {hi:9.3f}] PERMS {n / med * 1e3:.6e}")
        return 0
    n_cols, log2n, mode = int(rest[0]), int(rest[1]), rest[2]
    n = 1 << log2n
    t_cols = dev(inputs.rand_elems("stark252", n_cols * n, 42))
    t_nodes = torch.empty((2 * n - 1, 4), dtype=torch.int64, device="cuda")
    leaf = poseidon.LEAF_SINGLE if mode == "single" else poseidon.LEAF_MANY
    perms = n * (1 if mode == "single" else n_cols // 2 + 1) + n - 1
    med, lo, hi = timed(lambda: poseidon.commit_columns_device(t_cols, n_cols, log2n, t_nodes, leaf, True, return_root=False), reps=5)
    print(f"RESULT commit_columns_device {n_cols} x 2^{log2n} {mode}: {perms} permutations, {med:9.3f} ms [{lo:9.3f} .. {hi:9.3f}] PERMS {perms / med * 1e3:.6e}")
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "poseidon.txt"))
    ap.add_argument("--step")
    args = ap.parse_args()
    if args.step:
        return step(args.step)
    me = os.path.abspath(__file__)
    chain = " && ".join(f"timeout -k 10 {limit} {sys.executable} {me} --step {name}" for name, limit in STEPS)
    run = subprocess.run(chain, shell=True, capture_output=True, text=True, cwd=ROOT)
    lines = ["# Starknet Poseidon: wall ms per call, median [min .. max] after a warm-up (9 calls; 201 at 2^0; trees 5), stream synchronised"]
    ceiling = None
    for ln in run.stdout.splitlines():
        if ln.startswith("FE_MUL"):
            ceiling = float(ln.split()[1]) * 1e9 / PRODUCTS
            lines.append(f"{ln}; ceiling = rate / {PRODUCTS} = {ceiling:.4e} permutations/s")
        elif ln.startswith("RESULT"):
            rate = float(ln.rsplit("PERMS", 1)[1])
            lines.append(f"{ln[7:].rsplit('PERMS', 1)[0]}{rate:.4e} permutations/s"
                         + (f" = {rate / ceiling:.3f} of the {PRODUCTS}-product ceiling" if ceiling else ""))
    lines.append(f"# single CPU thread, DERIVED (not run): {CPU_NS_PER_PRODUCT:.1f} ns per Stark252 product (bench.py cpu_baseline leg, 2^24 evaluate_fft) "
                 f"x {PRODUCTS} = {CPU_NS_PER_PRODUCT * PRODUCTS / 1e3:.2f} us per permutation, {1e9 / (CPU_NS_PER_PRODUCT * PRODUCTS):.3e} permutations/s")
    if run.returncode:
        lines.append(f"# the chain stopped with exit status {run.returncode}: {run.stderr[-400:].strip()}")
    print("\n".join(lines), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return run.returncode


if __name__ == "__main__":
    sys.exit(main())
