#!/usr/bin/env python3
"""DEEP composition polynomial on the device, Stark252 (lw_stark_deep_composition_device): kernel time of the fused call
against the summed kernel time of the C * T + P lw_poly_ruffini_division_device calls that produce the individual
quotients of the same inputs.  That baseline is a lower bound on any composition from the division entry point: it leaves
out the weighted sum of the quotients and the host round trip.  Kernel times come from lw_hip_profile_* (HIP events around
every launch), after a warm-up call, as medians over --reps calls; min and max show the spread of the box.
Bytes counted for the fused call are the compulsory ones: (K * n reads + n writes) * 32.
usage: deep_composition_timing.py [--reps K] [--out FILE]"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from lambda_elliptic_curves_amd import _lib, fft, poly, stark  # noqa: E402

DEEP_KERNELS = ("deep_tile_reduce_kernel", "deep_tile_scan_kernel", "deep_tile_rescan_kernel")
DIV_KERNELS = ("poly_tile_reduce_kernel", "poly_tile_scan_kernel", "poly_tile_rescan_kernel")


def rand_stark(n, seed):
    """n canonical Stark252 elements (< 2^250 < p) on the device, (n, 4) int64"""
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    t = torch.randint(-(1 << 63), (1 << 63) - 1, (n, 4), dtype=torch.int64, device="cuda", generator=g)
    t[:, 0] &= (1 << 58) - 1
    return t


def profiled(fn, reps, names):
    """-> ([summed kernel ms per call], {kernel: median ms per call})"""
    fn()
    torch.cuda.synchronize()
    totals, kern = [], {}
    for _ in range(reps):
        _lib.profile_begin()
        fn()
        torch.cuda.synchronize()
        prof = _lib.profile_end()
        totals.append(sum(prof.get(k, (0, 0.0))[1] for k in names))
        for k in names:
            kern.setdefault(k, []).append(prof.get(k, (0, 0.0))[1])
    return totals, {k: statistics.median(v) for k, v in kern.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    F = fft.Stark252PrimeField
    z = np.array([0x123, 0x4567, 0x89ab, 0xcdef01], np.uint64)
    g = np.array([0x77, 0x1234567, 0x9abcdef, 0x13579b], np.uint64)
    gamma = np.array([0x1, 0xfedcba, 0x2468ac, 0xe02468], np.uint64)
    emit(f"# {torch.cuda.get_device_name(0)}, Stark252, reps = {args.reps}: median [min .. max] of the summed kernel time per call")
    emit("# fused = lw_stark_deep_composition_device (no host output); baseline = C*T + P lw_poly_ruffini_division_device calls")
    emit(f"{'C':>3} {'T':>2} {'P':>2} {'log2 n':>6} {'fused ms':>9} {'[min .. max]':>19} {'baseline ms':>11} {'[min .. max]':>19} "
         f"{'fused/base':>10} {'GB/s':>7}  fused per kernel")
    for C_, T, P_, lg in ((4, 3, 2, 20), (4, 3, 2, 22), (16, 3, 2, 20)):
        n, K = 1 << lg, C_ + P_
        t = [rand_stark(n, 1000 * lg + i) for i in range(K)]
        lens = [n] * K
        pts, w = stark.deep_terms(F, C_, P_, T, z, g, gamma)
        t_out = torch.empty((n - 1, 4), dtype=torch.int64, device="cuda")
        t_q = torch.empty((n - 1, 4), dtype=torch.int64, device="cuda")
        pairs = [(k, j) for k in range(K) for j in range(T + 1) if w[k, j].any()]
        assert len(pairs) == C_ * T + P_

        def fused():
            poly.deep_composition_device(F, t, lens, pts, w, t_out, evals=False)

        def baseline():
            for k, j in pairs:
                poly.ruffini_division_device(F, t[k], n, pts[j], t_q, remainder=False)

        tf, kf = profiled(fused, args.reps, DEEP_KERNELS)
        tb, _ = profiled(baseline, args.reps, DIV_KERNELS)
        mf, mb = statistics.median(tf), statistics.median(tb)
        per = ", ".join(f"{k.replace('deep_tile_', '').replace('_kernel', '')} {kf[k]:.3f}" for k in DEEP_KERNELS)
        emit(f"{C_:>3} {T:>2} {P_:>2} {lg:>6} {mf:9.3f} {'[%.3f .. %.3f]' % (min(tf), max(tf)):>19} {mb:11.3f} "
             f"{'[%.3f .. %.3f]' % (min(tb), max(tb)):>19} {mf / mb:10.3f} {(K + 1) * n * 32 / mf / 1e6:7.0f}  {per}")
        del t, t_out, t_q
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
