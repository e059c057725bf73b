#!/usr/bin/env python3
"""KZG opening on the device, BLS12-381 G1 (lw_kzg_open_device, lw_poly_*): kernel times of the division and the
evaluation at 2^16 .. 2^24 coefficients with their achieved bandwidth, and open against the SRS MSM of the same n - 1
scalars at 2^20, 2^22, 2^24, through a folded SRS handle (13 window-shifted copies, the default for large sets) and an
unfolded one.  Kernel times come from lw_hip_profile_* (HIP events around every launch); wall times are medians.
Bytes counted: division = 2 reads + 1 write of n elements, evaluation = 1 read.
usage: kzg_open_timing.py [--reps K] [--out FILE]"""
import argparse
import os
import statistics
import sys
import time

os.environ.setdefault("LW_HIP_TUNING", "1")   # LW_HIP_SRS_FOLD_MIN below is a tuning switch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from lambda_elliptic_curves_amd import _lib, fft, kzg, msm, poly  # noqa: E402
from tools.synth import distinct_points  # noqa: E402

POLY_KERNELS = ("poly_tile_reduce_kernel", "poly_tile_scan_kernel", "poly_tile_rescan_kernel")


def rand_fr(n, seed):
    """n canonical BLS12-381 Fr elements (< 2^254 < r) on the device, (n, 4) int64"""
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    t = torch.randint(-(1 << 63), (1 << 63) - 1, (n, 4), dtype=torch.int64, device="cuda", generator=g)
    t[:, 0] &= (1 << 62) - 1
    return t


def profiled(fn, reps):
    """-> (median wall ms, {kernel: median ms per call})"""
    fn()
    torch.cuda.synchronize()
    walls, kern = [], {}
    for _ in range(reps):
        _lib.profile_begin()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        walls.append((time.perf_counter() - t0) * 1e3)
        for k, (_, ms) in _lib.profile_end().items():
            kern.setdefault(k, []).append(ms)
    return statistics.median(walls), {k: statistics.median(v) for k, v in kern.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    F, crv = fft.FrField, msm.BLS12381Curve
    x = np.array([0, 0, 0x1234, 0x9abcdef], np.uint64)
    emit(f"# {torch.cuda.get_device_name(0)}, reps = {args.reps}, medians")
    emit("## kernels: division (reduce + scan + rescan) and evaluation (reduce + scan), one polynomial, one point")
    emit(f"{'log2 n':>6} {'div ms':>9} {'div GB/s':>9} {'eval ms':>9} {'eval GB/s':>9}  per kernel (division)")
    for lg in range(16, 25, 2):
        n = 1 << lg
        t = rand_fr(n, lg)
        tq = torch.empty((n - 1, 4), dtype=torch.int64, device="cuda")
        _, kd = profiled(lambda: poly.ruffini_division_device(F, t, n, x, tq, remainder=False), args.reps)
        _, ke = profiled(lambda: poly.evaluate_device(F, [t], [n], x), args.reps)
        d = sum(kd.get(k, 0.0) for k in POLY_KERNELS)
        e = sum(ke.get(k, 0.0) for k in POLY_KERNELS)
        per = ", ".join(f"{k.replace('poly_tile_', '').replace('_kernel', '')} {kd.get(k, 0.0):.3f}" for k in POLY_KERNELS)
        emit(f"{lg:>6} {d:9.3f} {3 * n * 32 / d / 1e6:9.0f} {e:9.3f} {n * 32 / e / 1e6:9.0f}  {per}")
        del t, tq

    top = 1 << 24
    pts = distinct_points(crv, top)
    for label, fold_min in (("folded", "19"), ("unfolded", "40")):
        os.environ["LW_HIP_SRS_FOLD_MIN"] = fold_min
        srs = msm.Srs(crv, t_points=pts, n=top)
        emit(f"## open vs msm_srs of the same n - 1 scalars, {label} SRS handle of 2^24 points")
        emit(f"{'log2 n':>6} {'open ms':>9} {'msm ms':>9} {'open/msm':>9} {'poly kern ms':>12} {'all kern ms':>11} {'poly share':>10}")
        for lg in (20, 22, 24):
            n = 1 << lg
            t = rand_fr(n, 100 + lg)
            tq = torch.empty((n - 1, 4), dtype=torch.int64, device="cuda")
            poly.ruffini_division_device(F, t, n, x, tq, remainder=False)
            w_open, k_open = profiled(lambda: kzg.open_device(srs, t, n, x), args.reps)
            w_msm, _ = profiled(lambda: srs.msm_device(tq, n - 1), args.reps)
            pk = sum(k_open.get(k, 0.0) for k in POLY_KERNELS)
            ak = sum(k_open.values())
            emit(f"{lg:>6} {w_open:9.2f} {w_msm:9.2f} {w_open / w_msm:9.3f} {pk:12.3f} {ak:11.2f} {100 * pk / ak:9.2f}%")
            del t, tq
        srs.close()
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
