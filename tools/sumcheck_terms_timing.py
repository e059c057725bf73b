#!/usr/bin/env python3
"""The eq table and the composed sumcheck round on the device (csrc/sumcheck_terms.hip): the eq table next to its two
ceilings, and the rounds of the Spartan-shaped proof eq (A B - C) next to what the product round alone offers for the same
claim.
  fe_mul     the Montgomery product rates of tools/microbench (built by build()), Stark252 and Fr381
  FIELD:LOG  for one field and table size 2^LOG, in one process:
             eq table   multilinear.eq_table_device of a random point, against (a) the output's bytes at the rate of a
                        device-to-device copy of the same size timed right there, (b) one product per element at the
                        fe_mul rate
             prove      the n rounds of the sumcheck of eq (A B - C): one composed round over (A, B, C) with the eq table
                        (sumcheck_terms_round_device, terms A B and - C; one plain round, then fused rounds) against two
                        product rounds a round, sumcheck_round_device of K = 3 over (eq, A, B) and of K = 2 over (a copy of
                        eq, C), with the same challenges, which are fixed in advance.  The round values of the two forms
                        are compared: g(u) = g3(u) - g2(u) for u = 0, 1, 2.  The tables are consumed, so each repetition
                        starts from a fresh copy (not timed).
Every step is a process of its own under `timeout -k 10`, chained with &&: a step that fails or hangs ends the run.
usage: sumcheck_terms_timing.py [--out FILE]        (sumcheck_terms_timing.py --step NAME runs one step)"""
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
REPS = 5


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


def to_int(x):
    import numpy as np
    return int.from_bytes(np.ascontiguousarray(x, dtype=np.uint64).astype(">u8").tobytes(), "big")


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
    p = multilinear.MODULI[F.field]
    dev = lambda a: torch.from_numpy(a.view(np.int64)).cuda()
    # the eq table and the copy of the same size, alternating
    tau = inputs.rand_elems(field, n, 60)
    t_eq = torch.empty((N, 4), dtype=torch.int64, device="cuda")
    dst = torch.empty_like(t_eq)
    eq, cp = [], []
    for _ in range(3):
        eq.append(timed(lambda: multilinear.eq_table_device(F, tau, t_eq)))
        cp.append(timed(lambda: dst.copy_(t_eq)))
    eq_med, cp_med = statistics.median(m for m, _, _ in eq), statistics.median(m for m, _, _ in cp)
    print(f"RESULT eq table {field} 2^{n}: {eq_med:8.3f} ms [{min(l for _, l, _ in eq):8.3f} .. {max(h for _, _, h in eq):8.3f}]; "
          f"copy of {N * 32 >> 20} MiB {cp_med:8.3f} ms [{min(l for _, l, _ in cp):8.3f} .. {max(h for _, _, h in cp):8.3f}] "
          f"EQ {field} {n} {eq_med:.6f} {cp_med:.6f}")
    # the rounds of eq (A B - C): composed against two product rounds, alternating
    master = [dev(inputs.rand_elems(field, N, 61 + k)) for k in range(3)] + [t_eq]
    work = [torch.empty_like(m) for m in master] + [torch.empty_like(t_eq)]   # A, B, C, eq, a second eq
    minus_one = np.frombuffer((p - (1 << 256) % p).to_bytes(32, "big"), dtype=">u8").astype(np.uint64)
    terms = [(None, (0, 1)), (minus_one, (2,))]
    rs = inputs.rand_elems(field, n, 70)
    tot = {"composed": [], "product": []}
    per = {"composed": [], "product": []}
    for rep in range(REPS + 1):   # the first repetition is the warm-up
        got = {}
        for form in ("composed", "product"):
            for k in range(4):
                work[k].copy_(master[k])
            work[4].copy_(t_eq)
            torch.cuda.synchronize()
            clock, rounds = [], []
            t_all = time.perf_counter()
            for i in range(n):
                nv, r = n - max(0, i - 1), (rs[i - 1] if i else None)
                t0 = time.perf_counter()
                if form == "composed":
                    g = multilinear.sumcheck_terms_round_device(F, work[:3], terms, nv, work[3], r)
                else:
                    g3 = multilinear.sumcheck_round_device(F, [work[3], work[0], work[1]], nv, r)
                    g2 = multilinear.sumcheck_round_device(F, [work[4], work[2]], nv, r)
                    g = (g3, g2)
                clock.append((time.perf_counter() - t0) * 1e3)
                rounds.append(g)
            torch.cuda.synchronize()
            if rep:
                tot[form].append((time.perf_counter() - t_all) * 1e3)
                per[form].append(clock)
            got[form] = rounds
        if rep == 0:
            for g, (g3, g2) in zip(got["composed"], got["product"]):
                if any(to_int(g[u]) != (to_int(g3[u]) - to_int(g2[u])) % p for u in range(3)):
                    print(f"the composed and the product rounds differ ({field}, 2^{n})")
                    return 1
    med = {f: statistics.median(tot[f]) for f in tot}
    print(f"RESULT prove eq (A B - C) {field} 2^{n}: composed {med['composed']:8.3f} ms [{min(tot['composed']):8.3f} .. {max(tot['composed']):8.3f}], "
          f"K = 3 round + K = 2 round {med['product']:8.3f} ms [{min(tot['product']):8.3f} .. {max(tot['product']):8.3f}], "
          f"product / composed = {med['product'] / med['composed']:.3f}; same round values")
    for f in ("composed", "product"):
        rounds = [statistics.median(c[i] for c in per[f]) for i in range(n)]
        print(f"RESULT   per round, {f:8s} (ms, median of {REPS}): " + " ".join(f"{v:.3f}" for v in rounds))
    big = [i for i in range(n) if n - i >= 18]   # the rounds over at least 2^18 elements, where the loads decide
    ratio = sum(statistics.median(c[i] for c in per["product"]) for i in big) / sum(statistics.median(c[i] for c in per["composed"]) for i in big)
    print(f"RESULT   rounds over 2^18 elements and more: product / composed = {ratio:.3f} (5 / 4 from the bytes alone)")
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sumcheck_terms.txt"))
    ap.add_argument("--step")
    args = ap.parse_args()
    if args.step:
        return step(args.step)
    me = os.path.abspath(__file__)
    chain = " && ".join(f"timeout -k 10 {limit} {sys.executable} {me} --step {name}" for name, limit in STEPS)
    run = subprocess.run(chain, shell=True, capture_output=True, text=True, cwd=ROOT)
    lines = [f"# eq table and composed sumcheck round: wall ms per call, median [min .. max] after a warm-up ({REPS} calls; eq table and "
             f"copy 3 x {REPS}, alternating), stream synchronised"]
    rate = {}
    for ln in run.stdout.splitlines():
        if ln.startswith("FE_MUL"):
            w = ln.split()
            rate = {w[1]: float(w[2]), w[3]: float(w[4])}
            lines.append(ln)
        elif ln.startswith("RESULT eq table"):
            head, tail = ln[7:].rsplit("EQ", 1)
            field, n, eq_ms, cp_ms = tail.split()
            eq_ms, cp_ms, N = float(eq_ms), float(cp_ms), 1 << int(n)
            gbs = 2 * N * 32 / cp_ms / 1e6
            c_mem = cp_ms / 2   # the output's bytes at the copy's read + write rate
            lines.append(head.rstrip())
            lines.append(f"    memory ceiling: copy at {gbs:.0f} GB/s read + write -> {c_mem:.3f} ms to write the table = {c_mem / eq_ms:.3f} of eq table")
            if field in rate:
                c_mul = N / rate[field] / 1e6
                lines.append(f"    product ceiling: {N} products at {rate[field]} Gmul/s -> {c_mul:.3f} ms = {c_mul / eq_ms:.3f} of eq table")
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
