#!/usr/bin/env python3
"""Multilinear tables on the device (csrc/multilinear.hip): evaluate next to its two ceilings, and a whole sumcheck proof
with fused rounds next to the same proof run as fix_variables plus a plain round.
  fe_mul     the Montgomery product rates of tools/microbench (built by build()), Stark252 and Fr381
  FIELD:LOG  for one field and table size 2^LOG, in one process:
             evaluate   multilinear.evaluate_device of one table, against (a) the table's bytes over the read + write rate of
                        a device-to-device copy of the same size timed right there, (b) one product per element at the
                        fe_mul rate
             prove      the n rounds of multilinear.sumcheck_prove_device for K = 2 and 3 (one plain round, then fused rounds,
                        the loop restated here so that every round has its own clock) against the same transcript produced
                        by sumcheck_round_device without r_prev and fix_variables_device of one variable per table between
                        two rounds (both forms synchronise once per round).  The tables are consumed, so each repetition
                        starts from a fresh copy (not timed).
Every step is a process of its own under `timeout -k 10`, chained with &&: a step that fails or hangs ends the run.
usage: multilinear_timing.py [--out FILE]        (multilinear_timing.py --step NAME runs one step)"""
import argparse
import os
import re
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STEPS = [("fe_mul", 240), ("stark252:20", 180), ("fr381:20", 180), ("stark252:24", 300), ("fr381:24", 300)]
REPS = 7


def timed(fn, reps=REPS):
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


def challenge(g):
    """a cheap stand-in for the caller's transcript: the last round value with its top limb cut below both moduli"""
    r = g[-1].copy()
    r[0] &= (1 << 59) - 1
    return r


def prove_unfused(multilinear, F, bufs, n, clock):
    """the transcript of sumcheck_prove_device from plain rounds and fix_variables between them; bufs[k] = (a, b) ping-pong"""
    import numpy as np
    cur = [a for a, _ in bufs]
    oth = [b for _, b in bufs]
    rounds = []
    for i in range(n):
        t0 = time.perf_counter()
        if i:
            for k in range(len(cur)):
                multilinear.fix_variables_device(F, cur[k], n - i + 1, r.reshape(1, 4), oth[k])
            cur, oth = oth, cur
        g = multilinear.sumcheck_round_device(F, cur, n - i)
        clock.append((time.perf_counter() - t0) * 1e3)
        rounds.append(g)
        r = challenge(g)
    return np.stack(rounds)


def prove_fused(multilinear, F, tabs, n, clock):
    import numpy as np
    rounds, r = [], None
    for i in range(n):
        t0 = time.perf_counter()
        g = multilinear.sumcheck_round_device(F, tabs, n - max(0, i - 1), r)
        clock.append((time.perf_counter() - t0) * 1e3)
        rounds.append(g)
        r = challenge(g)
    return np.stack(rounds)


def step(name):
    if name == "fe_mul":
        r = subprocess.run([os.path.join(ROOT, "tools", "microbench")], capture_output=True, text=True)
        m = dict(re.findall(r"RATE fe_mul (Stark252|Fr381)\s+([0-9.]+) Gmul/s", r.stdout))
        if r.returncode or len(m) != 2:
            print(r.stdout[-2000:] + r.stderr[-2000:])
            return 1
        print(f"FE_MUL stark252 {m['Stark252']} fr381 {m['Fr381']} Gmul/s (tools/microbench, fe_mul, all CUs)")
        return 0
    import numpy as np
    import torch
    from lambda_elliptic_curves_amd import multilinear
    from tools import inputs
    field, log = name.split(":")
    n = int(log)
    N = 1 << n
    F = inputs.field_pairs()[field][0]
    dev = lambda a: torch.from_numpy(a.view(np.int64)).cuda()
    master = [dev(inputs.rand_elems(field, N, 51 + k)) for k in range(3)]
    pt = inputs.rand_elems(field, n, 50)
    # evaluate and the copy of the same size, alternating
    dst = torch.empty_like(master[0])
    ev, cp = [], []
    for _ in range(3):
        ev.append(timed(lambda: multilinear.evaluate_device(F, master[:1], n, pt)))
        cp.append(timed(lambda: dst.copy_(master[0])))
    ev_med, cp_med = statistics.median(m for m, _, _ in ev), statistics.median(m for m, _, _ in cp)
    print(f"RESULT evaluate {field} 2^{n}: {ev_med:8.3f} ms [{min(l for _, l, _ in ev):8.3f} .. {max(h for _, _, h in ev):8.3f}]; "
          f"copy of {N * 32 >> 20} MiB {cp_med:8.3f} ms [{min(l for _, l, _ in cp):8.3f} .. {max(h for _, _, h in cp):8.3f}] "
          f"EVAL {field} {n} {ev_med:.6f} {cp_med:.6f}")
    # the whole proof, fused against unfused, alternating
    work = [(torch.empty_like(m), torch.empty((N // 2, 4), dtype=torch.int64, device="cuda")) for m in master]
    for K in (2, 3):
        tot = {"fused": [], "unfused": []}
        per = {"fused": [], "unfused": []}
        same = True
        for rep in range(REPS + 1):   # the first repetition is the warm-up
            got = {}
            for form in ("fused", "unfused"):
                for k in range(K):
                    work[k][0].copy_(master[k])
                torch.cuda.synchronize()
                clock = []
                t0 = time.perf_counter()
                if form == "fused":
                    got[form] = prove_fused(multilinear, F, [work[k][0] for k in range(K)], n, clock)
                else:
                    got[form] = prove_unfused(multilinear, F, work[:K], n, clock)
                torch.cuda.synchronize()
                if rep:
                    tot[form].append((time.perf_counter() - t0) * 1e3)
                    per[form].append(clock)
            same = same and np.array_equal(got["fused"], got["unfused"])
        if not same:
            print(f"the fused and unfused transcripts differ ({field}, 2^{n}, K = {K})")
            return 1
        med = {f: statistics.median(tot[f]) for f in tot}
        print(f"RESULT prove {field} 2^{n} K = {K}: fused {med['fused']:8.3f} ms [{min(tot['fused']):8.3f} .. {max(tot['fused']):8.3f}], "
              f"fix_variables + plain round {med['unfused']:8.3f} ms [{min(tot['unfused']):8.3f} .. {max(tot['unfused']):8.3f}], "
              f"unfused / fused = {med['unfused'] / med['fused']:.3f}; same transcript")
        for f in ("fused", "unfused"):
            rounds = [statistics.median(c[i] for c in per[f]) for i in range(n)]
            print(f"RESULT   per round, {f:7s} (ms, median of {REPS}): " + " ".join(f"{v:.3f}" for v in rounds))
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "multilinear.txt"))
    ap.add_argument("--step")
    args = ap.parse_args()
    if args.step:
        return step(args.step)
    me = os.path.abspath(__file__)
    chain = " && ".join(f"timeout -k 10 {limit} {sys.executable} {me} --step {name}" for name, limit in STEPS)
    run = subprocess.run(chain, shell=True, capture_output=True, text=True, cwd=ROOT)
    lines = [f"# multilinear tables: wall ms per call, median [min .. max] after a warm-up ({REPS} calls; evaluate and copy 3 x {REPS}, "
             "alternating), stream synchronised"]
    rate = {}
    for ln in run.stdout.splitlines():
        if ln.startswith("FE_MUL"):
            w = ln.split()
            rate = {w[1]: float(w[2]), w[3]: float(w[4])}
            lines.append(ln)
        elif ln.startswith("RESULT evaluate"):
            head, tail = ln[7:].rsplit("EVAL", 1)
            field, n, ev_ms, cp_ms = tail.split()
            ev_ms, cp_ms, N = float(ev_ms), float(cp_ms), 1 << int(n)
            gbs = 2 * N * 32 / cp_ms / 1e6
            c_mem = cp_ms / 2   # the table's bytes at the copy's read + write rate
            lines.append(head.rstrip())
            lines.append(f"    memory ceiling: copy at {gbs:.0f} GB/s read + write -> {c_mem:.3f} ms to read the table = {c_mem / ev_ms:.3f} of evaluate")
            if field in rate:
                c_mul = N / rate[field] / 1e6
                lines.append(f"    product ceiling: {N} products at {rate[field]} Gmul/s -> {c_mul:.3f} ms = {c_mul / ev_ms:.3f} of evaluate")
        elif ln.startswith("RESULT"):
            lines.append(ln[7:])
    if run.returncode:
        lines.append(f"# the chain stopped with exit status {run.returncode}: {(run.stdout[-400:] + run.stderr[-400:]).strip()}")
    print("\n".join(lines), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return run.returncode


if __name__ == "__main__":
    sys.exit(main())
