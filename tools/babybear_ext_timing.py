#!/usr/bin/env python3
"""The BabyBear quartic extension on the device (csrc/babybear_ext.hip), every new kernel next to a device copy of the
bytes it moves, and one FRI layer next to its parts called one by one, all timed in the same process.
  pointwise  mul and inv over 2^24 elements against a copy of the planes read and written
  evaluate   8 columns of 2^20 coefficients at 3 points against a copy of the columns (the call waits for its values)
  deep       8 columns of 2^22 rows, 3 points against a copy of the columns read and the four planes written
  layer      2^20 Fp4 coefficients -> block 2^19, domain 2^21, Keccak tree, against the sum of its parts called one by
             one: fold only, fft.lde_device with batch = 4, and merkle.commit_columns_layout_device over the evaluation as
             eight columns of half a plane (the layer's tree is no call of its own; this one hashes the same 32 bytes per
             leaf in another order and builds the same levels above them); the fold against a copy
  kernels    device time of every kernel of one call of each (lw_hip_profile_begin / end), a run of its own
Every step is a process of its own under `timeout -k 10`; the first step that fails or hangs ends the run.
usage: babybear_ext_timing.py [--out FILE]        (babybear_ext_timing.py --step NAME runs one step)"""
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
LOG_POINTWISE, LOG_COEFFS, LOG_DOMAIN, COLUMNS, POINTS = 24, 20, 22, 8, 3


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
    return torch.from_numpy(inputs.rand_elems("babybear_u32", count, seed).view("int32")).cuda()


def copy_of(n_words):
    """a device copy that reads and writes n_words / 2 words each: the traffic of a kernel that moves n_words"""
    import torch
    src = torch.zeros(n_words // 2, dtype=torch.int32, device="cuda")
    dst = torch.empty_like(src)
    return lambda: dst.copy_(src)


def fmt(t):
    return f"{t[0]:8.4f} ms [{t[1]:8.4f} .. {t[2]:8.4f}]"


def report(label, shape, t, c, moved_words):
    ratio = t[0] / c[0]
    spread = ratio * ((t[2] - t[1]) / (2 * t[0]) + (c[2] - c[1]) / (2 * c[0]))
    print(f"RESULT {label:<12} {shape:<28} {fmt(t)}   copy of {moved_words * 4 / 2**20:7.1f} MiB moved {fmt(c)}   call / copy = {ratio:.2f} +- {spread:.2f}")


def points(count, seed):
    from tools import inputs
    w = inputs.rand_elems("babybear_u32", 4 * count, seed)
    return [(int(w[4 * j]), int(w[4 * j + 1]), int(w[4 * j + 2]), int(w[4 * j + 3]) or 1) for j in range(count)]


def layer_calls():
    """the layer, fold only, and its parts on preallocated buffers"""
    import numpy as np
    import torch
    from lambda_elliptic_curves_amd import _lib as L
    from lambda_elliptic_curves_amd import fft, merkle
    from lambda_elliptic_curves_amd.errors import check
    from tools import inputs
    n, block, domain = 1 << LOG_COEFFS, 1 << (LOG_COEFFS - 1), 1 << (LOG_DOMAIN - 1)
    t_coeffs = words(4 * n, 11)
    t_poly, t_eval = torch.empty(4 * block, dtype=torch.int32, device="cuda"), torch.empty(4 * domain, dtype=torch.int32, device="cuda")
    t_nodes = torch.empty((domain - 1, 32), dtype=torch.uint8, device="cuda")
    zeta, off, root = np.array(points(1, 12)[0], np.uint32), inputs.offset_elem("babybear_u32", 49), np.zeros(32, np.uint8)
    lib = L.lib()
    u32 = fft.Babybear31PrimeFieldU32

    def layer():
        check(lib.lw_babybear_ext4_fri_layer_device(L.device_ptr(t_coeffs), 0, n, L.host_ptr(zeta), L.host_ptr(off), domain, L.device_ptr(t_poly),
                                                    L.device_ptr(t_eval), L.device_ptr(t_nodes), L.host_ptr(root), L.stream_ptr(None)))

    def fold():
        check(lib.lw_babybear_ext4_fri_layer_device(L.device_ptr(t_coeffs), 0, n, L.host_ptr(zeta), None, 0, L.device_ptr(t_poly), None, None, None,
                                                    L.stream_ptr(None)))

    lde = lambda: fft.lde_device(u32, t_poly, LOG_COEFFS - 1, t_eval, LOG_DOMAIN - 1, batch=4, offset=off)
    # eight columns of half a plane each: the leaves hash the same 32 bytes as the layer's, (c0[i], c0[i + N/2], c1[i], ...)
    commit = lambda: merkle.commit_columns_layout_device(u32, t_eval, 8, LOG_DOMAIN - 2, t_nodes)
    return layer, fold, lde, commit


def step(name):
    import torch
    from lambda_elliptic_curves_amd import _lib
    from lambda_elliptic_curves_amd import babybear_ext as E
    from tools import inputs
    n, rows, big = 1 << LOG_COEFFS, 1 << LOG_DOMAIN, 1 << LOG_POINTWISE
    pts = points(POINTS, 5)
    h = int(inputs.offset_elem("babybear_u32", 7)[0])
    if name == "pointwise":
        t_a, t_b, t_out = words(4 * big, 1), words(4 * big, 2), torch.empty(4 * big, dtype=torch.int32, device="cuda")
        for label, op, moved in (("mul", E.MUL, 12 * big), ("inv", E.INV, 8 * big)):
            t = timed(lambda: E.pointwise_device(op, t_a, t_b, t_out, big))
            report(label, f"2^{LOG_POINTWISE} elements", t, timed(copy_of(moved)), moved)
        return 0
    if name == "evaluate":
        t_cols = words(COLUMNS * n, 3)
        t = timed(lambda: E.evaluate_device(t_cols, COLUMNS, n, pts))
        report("evaluate", f"{COLUMNS} x 2^{LOG_COEFFS}, {POINTS} points", t, timed(copy_of(COLUMNS * n)), COLUMNS * n)
        return 0
    if name == "deep":
        t_cols, t_out = words(COLUMNS * rows, 4), torch.empty(4 * rows, dtype=torch.int32, device="cuda")
        tab = [points(POINTS, 20 + k) for k in range(COLUMNS)]
        t = timed(lambda: E.deep_quotients_device(t_cols, COLUMNS, LOG_DOMAIN, pts, tab, tab, t_out, offset=h))
        report("deep", f"{COLUMNS} x 2^{LOG_DOMAIN}, {POINTS} points", t, timed(copy_of((COLUMNS + 4) * rows)), (COLUMNS + 4) * rows)
        return 0
    layer, fold, lde, commit = layer_calls()
    if name == "layer":
        tl, tf, te, tc = timed(layer), timed(fold), timed(lde), timed(commit)
        parts = tf[0] + te[0] + tc[0]
        spread = sum((x[2] - x[1]) / 2 for x in (tf, te, tc))
        shape = f"2^{LOG_COEFFS} -> 2^{LOG_COEFFS - 1} on 2^{LOG_DOMAIN - 1}"
        print(f"RESULT layer        {shape:<28} {fmt(tl)}   parts: fold {fmt(tf)} + lde batch 4 {fmt(te)} + keccak commit 8 columns {fmt(tc)} = {parts:8.4f} ms +- {spread:.4f}"
              f"   layer / parts = {tl[0] / parts:.3f}")
        report("fold", f"2^{LOG_COEFFS} -> 2^{LOG_COEFFS - 1}", tf, timed(copy_of(6 * n)), 6 * n)
        return 0
    # kernels: one call of each under the library's profiler
    t_a, t_out = words(COLUMNS * rows, 4), torch.empty(4 * big, dtype=torch.int32, device="cuda")
    t_b = words(4 * big, 2)
    tab = [points(POINTS, 20 + k) for k in range(COLUMNS)]
    calls = [("pointwise mul", lambda: E.pointwise_device(E.MUL, t_b, t_b, t_out, big)),
             ("pointwise inv", lambda: E.pointwise_device(E.INV, t_b, None, t_out, big)),
             ("evaluate", lambda: E.evaluate_device(t_a, COLUMNS, n, pts)),
             ("deep", lambda: E.deep_quotients_device(t_a, COLUMNS, LOG_DOMAIN, pts, tab, tab, t_out, offset=h)),
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "babybear_ext.txt"))
    ap.add_argument("--step")
    args = ap.parse_args()
    if args.step:
        return step(args.step)
    me = os.path.abspath(__file__)
    lines = [f"# BabyBear quartic extension: wall ms per call, median [min .. max] of {SAMPLES} samples of {CALLS} calls enqueued back to back after a",
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
