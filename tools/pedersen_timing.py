#!/usr/bin/env python3
"""Starknet Pedersen hash on the device (csrc/pedersen.hip): hashes per second next to the ceiling the arithmetic sets.
  fe_mul     the Stark252 Montgomery product rate of tools/microbench (built by build()); rate / PRODUCTS is the ceiling
  hash       pedersen.hash_device at 2^16 and 2^20 random pairs; one pair through hash_device and through hash (the call itself)
  tree       pedersen.commit_leaves_device over 2^20 leaf values (2^20 - 1 hashes)
  resources  VGPRs, SGPRs, scratch and occupancy of every kernel of pedersen.hip, from the compiler's resource-usage
             remarks (a compile for gfx950, no device involved)
Every step is a process of its own under `timeout -k 10`, chained with &&: a step that fails or hangs ends the run.
usage: pedersen_timing.py [--out FILE]        (pedersen_timing.py --step NAME runs one step)"""
import argparse
import os
import re
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# Counted products of one hash of uniform inputs below p (csrc/pedersen.cuh):
#   additions   a value has 62 low nibbles, each non-zero with probability 15/16, and bits 248 .. 251, which are 0 .. 7 for all
#               but 2^-55 of the values, non-zero with probability 7/8: 2 x (62 x 15/16 + 7/8) = 118.0 on average, 126 at most
#   products    11 per mixed Jacobian addition (8 M + 3 S)
#   the rest    2 (both inputs out of Montgomery form) + 2 (the shift point into it) + 2 (Z^-2, X Z^-2) + 2 inside fe_inv_fast
# The binary GCD of fe_inv_fast itself is VALU work that is not a product and is NOT in the count: the ceiling is that much
# too high.
ADDS, PER_ADD, REST = 118.0, 11, 8
PRODUCTS = ADDS * PER_ADD + REST
# a trailing ":host" times the host form (staged, complete on return); at 2^0 a line is the cost of the call itself
STEPS = [("fe_mul", 240), ("hash:0", 120), ("hash:0:host", 120), ("hash:16", 120), ("hash:20", 120), ("tree:20", 180), ("resources", 300)]


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


def resources():
    csrc = os.path.join(ROOT, "lambda_elliptic_curves_amd", "csrc")
    with tempfile.TemporaryDirectory() as tmp:
        r = subprocess.run(["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-Rpass-analysis=kernel-resource-usage",
                            "-c", os.path.join(csrc, "pedersen.hip"), "-o", os.path.join(tmp, "pedersen.o")], capture_output=True, text=True)
    if r.returncode:
        print(r.stderr[-2000:])
        return 1
    cur = {}
    for ln in r.stderr.splitlines():
        m = re.search(r"remark:\s+(Function Name|TotalSGPRs|VGPRs|AGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|LDS Size \[bytes/block\]): (\S+)", ln)
        if not m:
            continue
        if m.group(1) == "Function Name":
            cur = {"name": m.group(2)}
        else:
            cur[m.group(1).split(" ")[0]] = m.group(2)
        if m.group(1).startswith("LDS"):
            # _ZN2lw<len><kernel>[INS_<len><policy>E...]: the kernel and its hash policy out of the mangled name
            m = re.match(r"_ZN2lw\d+?([a-z_]+)(?:INS_(\d+)([A-Za-z]+))?", cur["name"])
            name = (m.group(1) + (f"<{m.group(3)[:int(m.group(2))]}>" if m.group(2) else "")) if m else cur["name"]
            print(f"KERNEL {name}: {cur['VGPRs']} VGPRs, {cur['AGPRs']} AGPRs, {cur['TotalSGPRs']} SGPRs, scratch {cur['ScratchSize']} bytes/lane, "
                  f"LDS {cur['LDS']} bytes, occupancy {cur['Occupancy']} waves/SIMD")
    return 0


def step(name):
    if name == "fe_mul":
        r = subprocess.run([os.path.join(ROOT, "tools", "microbench")], capture_output=True, text=True)
        m = re.search(r"RATE fe_mul Stark252\s+([0-9.]+) Gmul/s", r.stdout)
        if r.returncode or not m:
            print(r.stdout[-2000:] + r.stderr[-2000:])
            return 1
        print(f"FE_MUL {m.group(1)} Gmul/s (tools/microbench, fe_mul Stark252, all CUs)")
        return 0
    if name == "resources":
        return resources()
    import numpy as np
    import torch
    from lambda_elliptic_curves_amd import pedersen
    from tools import inputs
    dev = lambda a: torch.from_numpy(a.view(np.int64)).cuda()
    kind, log2n, *host = name.split(":")
    n = 1 << int(log2n)
    if kind == "hash":
        x, y = inputs.rand_elems("stark252", n, 41), inputs.rand_elems("stark252", n, 42)
        t_x, t_y = dev(x), dev(y)
        t_out = torch.empty((n, 4), dtype=torch.int64, device="cuda")
        med, lo, hi = timed((lambda: pedersen.hash(x, y)) if host else (lambda: pedersen.hash_device(t_x, t_y, n, t_out)), reps=201 if n == 1 else 9)
        print(f"RESULT hash{'' if host else '_device'} 2^{log2n}: {n} hashes, {med:9.3f} ms [{lo:9.3f} .. {hi:9.3f}] HASHES {n / med * 1e3:.6e}")
        return 0
    t_leaves = dev(inputs.rand_elems("stark252", n, 43))
    t_nodes = torch.empty((2 * n - 1, 4), dtype=torch.int64, device="cuda")
    med, lo, hi = timed(lambda: pedersen.commit_leaves_device(t_leaves, int(log2n), t_nodes, True, return_root=False), reps=5)
    print(f"RESULT commit_leaves_device 2^{log2n}: {n - 1} hashes, {med:9.3f} ms [{lo:9.3f} .. {hi:9.3f}] HASHES {(n - 1) / med * 1e3:.6e}")
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pedersen.txt"))
    ap.add_argument("--step")
    args = ap.parse_args()
    if args.step:
        return step(args.step)
    me = os.path.abspath(__file__)
    chain = " && ".join(f"timeout -k 10 {limit} {sys.executable} {me} --step {name}" for name, limit in STEPS)
    run = subprocess.run(chain, shell=True, capture_output=True, text=True, cwd=ROOT)
    lines = ["# Starknet Pedersen hash: wall ms per call, median [min .. max] after a warm-up (9 calls; 201 at 2^0; the tree 5), stream synchronised",
             f"# counted products per hash of uniform inputs: {ADDS:.1f} additions (2 x (62 x 15/16 + 7/8); 126 at most) x {PER_ADD} (8 M + 3 S, mixed Jacobian) "
             f"+ {REST} (Montgomery form in and out of the nibbles, the shift point, Z^-2 and X Z^-2, 2 inside fe_inv_fast) = {PRODUCTS:.0f};",
             "# the binary GCD of the one inversion per hash is VALU work outside the count, so the ceiling below is that much too high",
             "# one inversion per hash (fe_inv_fast); Montgomery's trick across a workgroup: NOT MEASURED (not built)",
             "# table lookups by global loads; an LDS-staged flat kernel: NOT MEASURED (not built)"]
    ceiling = None
    for ln in run.stdout.splitlines():
        if ln.startswith("FE_MUL"):
            ceiling = float(ln.split()[1]) * 1e9 / PRODUCTS
            lines.append(f"{ln}; ceiling = rate / {PRODUCTS:.0f} = {ceiling:.4e} hashes/s")
        elif ln.startswith("RESULT"):
            rate = float(ln.rsplit("HASHES", 1)[1])
            lines.append(f"{ln[7:].rsplit('HASHES', 1)[0]}{rate:.4e} hashes/s" + (f" = {rate / ceiling:.3f} of the {PRODUCTS:.0f}-product ceiling" if ceiling else ""))
        elif ln.startswith("KERNEL"):
            lines.append(ln[7:])
    if run.returncode:
        lines.append(f"# the chain stopped with exit status {run.returncode}: {run.stderr[-400:].strip()}; what is missing above was NOT MEASURED")
    print("\n".join(lines), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return run.returncode


if __name__ == "__main__":
    sys.exit(main())
