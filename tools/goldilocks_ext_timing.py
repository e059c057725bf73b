#!/usr/bin/env python3
"""The Goldilocks quadratic extension on the device (csrc/goldilocks_ext.hip), every new kernel next to a device copy of
the bytes it moves, and one FRI layer next to its parts called one by one, all timed in the same process.
Sizes: 2^20 coefficients, an LDE domain of 2^22, 8 trace columns, 3 points.
  pointwise  mul / sqr / inv / mul_base over 2^22 elements against a copy of the planes read and written
  evaluate   8 columns of 2^20 coefficients at 3 points against a copy of the columns (the call waits for its values)
  deep       8 columns of 2^22 rows, 3 points against a copy of the columns read and the two planes written
  layer      2^20 Fp2 coefficients -> block 2^19, domain 2^21, RPO-128 tree, against the sum of fold only,
             goldilocks.lde_device with batch = 2 and rpo.commit_columns_device over four columns; the fold against a copy
  kernels    device time of every kernel of one call of each (lw_hip_profile_begin / end), a run of its own
Every step is a process of its own under `timeout -k 10`; the first step that fails or hangs ends the run.
usage: goldilocks_ext_timing.py [--out FILE]        (goldilocks_ext_timing.py --step NAME runs one step)"""
import argparse
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STEPS = [("pointwise", 180), ("evaluate", 180), ("deep", 180), ("layer", 240), ("kernels", 240)]
CALLS, SAMPLES = 10, 9
LOG_COEFFS, LOG_DOMAIN, COLUMNS, POINTS = 20, 22, 8, 3


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
    import torch
    from tools import inputs
    return torch.from_numpy(inputs.rand_elems("goldilocks", count, seed).view("int64")).cuda()


def copy_of(n_words):
    """a device copy that reads and writes n_words / 2 words each: the traffic of a kernel that moves n_words"""
    import torch
    src = torch.zeros(n_words // 2, dtype=torch.int64, device="cuda")
    dst = torch.empty_like(src)
    return lambda: dst.copy_(src)


def fmt(t):
    return f"{t[0]:8.4f} ms [{t[1]:8.4f} .. {t[2]:8.4f}]"


def report(label, shape, t, c, moved_words):
    ratio = t[0] / c[0]
    spread = ratio * ((t[2] - t[1]) / (2 * t[0]) + (c[2] - c[1]) / (2 * c[0]))
    print(f"RESULT {label:<12} {shape:<28} {fmt(t)}   copy of {moved_words * 8 / 2**20:7.1f} MiB moved {fmt(c)}   call / copy = {ratio:.2f} +- {spread:.2f}")


def points(count, seed):
    from tools import inputs
    w = inputs.rand_elems("goldilocks", 2 * count, seed)
    return [(int(w[2 * j]), int(w[2 * j + 1]) or 1) for j in range(count)]


def layer_calls():
    """the layer, fold only, and its parts on preallocated buffers, each returning after the stream has been waited for"""
    import numpy as np
    import torch
    from lambda_elliptic_curves_amd import _lib as L
    from lambda_elliptic_curves_amd import goldilocks, rpo
    from lambda_elliptic_curves_amd import goldilocks_ext as E
    from lambda_elliptic_curves_amd.errors import check
    n, block, domain = 1 << LOG_COEFFS, 1 << (LOG_COEFFS - 1), 1 << (LOG_DOMAIN - 1)
    t_coeffs = words(2 * n, 11)
    t_poly, t_eval = torch.empty(2 * block, dtype=torch.int64, device="cuda"), torch.empty(2 * domain, dtype=torch.int64, device="cuda")
    t_nodes = torch.empty((domain - 1) * 4, dtype=torch.int64, device="cuda")
    zeta, off, root = np.array(points(1, 12)[0], np.uint64), np.array([49], np.uint64), np.zeros(4, np.uint64)
    lib = L.lib()

    def layer():
        check(lib.lw_goldilocks_ext2_fri_layer_device(L.device_ptr(t_coeffs), 0, n, L.host_ptr(zeta), L.host_ptr(off), domain, 0, E.RPO_128,
                                                      L.device_ptr(t_poly), L.device_ptr(t_eval), L.device_ptr(t_nodes), L.host_ptr(root), L.stream_ptr(None)))

    def fold():
        check(lib.lw_goldilocks_ext2_fri_layer_device(L.device_ptr(t_coeffs), 0, n, L.host_ptr(zeta), None, 0, 0, E.RPO_128, L.device_ptr(t_poly),
                                                      None, None, None, L.stream_ptr(None)))

    lde = lambda: goldilocks.lde_device(t_poly, LOG_COEFFS - 1, t_eval, LOG_DOMAIN - 1, batch=2, offset=49)
    commit = lambda: rpo.commit_columns_device(rpo.LEVEL_128, t_eval, 4, LOG_DOMAIN - 2, t_nodes, col_stride=domain // 2)
    return layer, fold, lde, commit


def step(name):
    import torch
    from lambda_elliptic_curves_amd import _lib
    from lambda_elliptic_curves_amd import goldilocks_ext as E
    n, rows = 1 << LOG_COEFFS, 1 << LOG_DOMAIN
    pts = points(POINTS, 5)
    if name == "pointwise":
        t_a, t_b, t_out = words(2 * rows, 1), words(2 * rows, 2), torch.empty(2 * rows, dtype=torch.int64, device="cuda")
        for label, op, moved in (("mul", E.MUL, 6 * rows), ("sqr", E.SQR, 4 * rows), ("inv", E.INV, 4 * rows), ("mul_base", E.MUL_BASE, 5 * rows)):
            t = timed(lambda: E.pointwise_device(op, t_a, t_b, t_out, rows))
            report(label, f"2^{LOG_DOMAIN} elements", t, timed(copy_of(moved)), moved)
        return 0
    if name == "evaluate":
        t_cols = words(COLUMNS * n, 3)
        t = timed(lambda: E.evaluate_device(t_cols, COLUMNS, n, pts))
        report("evaluate", f"{COLUMNS} x 2^{LOG_COEFFS}, {POINTS} points", t, timed(copy_of(COLUMNS * n)), COLUMNS * n)
        return 0
    if name == "deep":
        t_cols, t_out = words(COLUMNS * rows, 4), torch.empty(2 * rows, dtype=torch.int64, device="cuda")
        tab = [points(POINTS, 20 + k) for k in range(COLUMNS)]
        t = timed(lambda: E.deep_quotients_device(t_cols, COLUMNS, LOG_DOMAIN, pts, tab, tab, t_out, offset=7))
        report("deep", f"{COLUMNS} x 2^{LOG_DOMAIN}, {POINTS} points", t, timed(copy_of((COLUMNS + 2) * rows)), (COLUMNS + 2) * rows)
        return 0
    layer, fold, lde, commit = layer_calls()
    if name == "layer":
        tl, tf, te, tc = timed(layer), timed(fold), timed(lde), timed(commit)
        parts = tf[0] + te[0] + tc[0]
        spread = sum((x[2] - x[1]) / 2 for x in (tf, te, tc))
        shape = f"2^{LOG_COEFFS} -> 2^{LOG_COEFFS - 1} on 2^{LOG_DOMAIN - 1}"
        print(f"RESULT layer        {shape:<28} {fmt(tl)}   parts: fold {fmt(tf)} + lde batch 2 {fmt(te)} + rpo commit 4 columns {fmt(tc)} = {parts:8.4f} ms +- {spread:.4f}"
              f"   layer / parts = {tl[0] / parts:.3f}")
        report("fold", f"2^{LOG_COEFFS} -> 2^{LOG_COEFFS - 1}", tf, timed(copy_of(3 * n)), 3 * n)
        return 0
    # kernels: one call of each under the library's profiler
    t_cols, t_out = words(COLUMNS * rows, 4), torch.empty(2 * rows, dtype=torch.int64, device="cuda")
    tab = [points(POINTS, 20 + k) for k in range(COLUMNS)]
    calls = [("pointwise mul", lambda: E.pointwise_device(E.MUL, t_cols, t_cols[2 * rows:], t_out, rows)),
             ("pointwise inv", lambda: E.pointwise_device(E.INV, t_cols, None, t_out, rows)),
             ("evaluate", lambda: E.evaluate_device(t_cols, COLUMNS, n, pts)),
             ("deep", lambda: E.deep_quotients_device(t_cols, COLUMNS, LOG_DOMAIN, pts, tab, tab, t_out, offset=7)),
             ("layer", layer)]
    for label, fn in calls:
        fn()
        torch.cuda.synchronize()
        _lib.profile_begin()
        for _ in range(CALLS):
            fn()
        torch.cuda.synchronize()
        for kname, (launches, ms) in sorted(_lib.profile_end().items()):
            print(f"KERNEL {label:<14} {kname:<24} {launches / CALLS:g} per call  {ms / launches:8.4f} ms each")
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "goldilocks_ext.txt"))
    ap.add_argument("--step")
    args = ap.parse_args()
    if args.step:
        return step(args.step)
    me = os.path.abspath(__file__)
    lines = [f"# Goldilocks quadratic extension: wall ms per call, median [min .. max] of {SAMPLES} samples of {CALLS} calls enqueued back to back after a",
             "# warm-up, stream synchronised; a copy is torch's device-to-device copy of half the words the call moves (read once, written once);",
             "# the spread beside a ratio is the half range of both sides.  KERNEL lines: device time between events, from a run of its own."]
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
