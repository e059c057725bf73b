#!/usr/bin/env python3
"""PLONK rounds 2 and 3 on the device (lw_plonk_round2_device, lw_plonk_round3_device) over BLS12-381 Fr at n = 2^16 and
2^20: wall time (median, min, max) and the kernel time from lw_hip_profile_* (HIP events around every launch), summed
and per kernel.  Beside them, in the same process, what a caller had before the rounds existed:
  transforms only   16 coset evaluations of 4n points and one inverse through lw_hip_ntt_device (zero-padded 4n inputs
                    already on the device), nothing in between;
  host buffers      the 17 evaluate_offset_fft calls and the interpolate_offset_fft of the reference's round 3 through
                    the host-buffer entry points, transfers included, again nothing in between.
Both baselines leave out the element-wise passes, so they are lower bounds of the old flow.
The inputs are random field elements: the rounds are arithmetic on whatever they are given.
usage: plonk_rounds_timing.py [--reps K] [--host-reps K] [--out FILE]"""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from lambda_elliptic_curves_amd import _lib, fft, plonk  # noqa: E402
from tools import inputs  # noqa: E402


def timed(fn, reps, profile=True):
    """-> (median, min, max wall ms, {kernel: (median ms per call, launches)})"""
    for _ in range(2):   # warm-up: tables, workspaces, clocks
        fn()
    torch.cuda.synchronize()
    walls, kern, cnt = [], {}, {}
    for _ in range(reps):
        if profile:
            _lib.profile_begin()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        walls.append((time.perf_counter() - t0) * 1e3)
        if profile:
            for k, (launches, ms) in _lib.profile_end().items():
                kern.setdefault(k, []).append(ms)
                cnt[k] = launches
    return statistics.median(walls), min(walls), max(walls), {k: (statistics.median(v), cnt[k]) for k, v in kern.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    F = fft.FrField
    k1 = inputs.offset_elem("fr381", 7)
    emit(f"# {torch.cuda.get_device_name(0)}, BLS12-381 Fr, reps = {args.reps} (host-buffer baseline: {args.host_reps}), wall = median [min, max] ms")
    for lg in (16, 20):
        n = 1 << lg
        el = lambda count, seed: inputs.rand_elems("fr381", count, seed)
        t0 = time.perf_counter()
        cir = plonk.Circuit(F, n, k1, [el(n, 10 + j) for j in range(5)], [el(n, 20 + j) for j in range(3)], [el(n, 30 + j) for j in range(3)])
        emit(f"## n = 2^{lg}: circuit handle built in {(time.perf_counter() - t0) * 1e3:.1f} ms (uploads included), {1376 * n / 2**20:.0f} MiB resident")
        t_w = torch.from_numpy(el(3 * n, 1).view(np.int64)).cuda()
        beta, gamma, alpha = el(1, 2)[0], el(1, 3)[0], el(1, 4)[0]
        bl3, bl2, pub = el(3, 5), el(2, 6), el(8, 7)
        t_abc = cir.round1_device(t_w, el(6, 8))
        t_z = cir.round2_device(t_w, beta, gamma, bl3)
        results = {}
        for name, fn in (("round 2", lambda: cir.round2_device(t_w, beta, gamma, bl3)),
                         ("round 3", lambda: cir.round3_device(t_abc, t_z, pub, beta, gamma, alpha, bl2))):
            med, lo, hi, kern = timed(fn, args.reps)
            ksum = sum(ms for ms, _ in kern.values())
            results[name] = (med, ksum)
            emit(f"{name}: wall {med:.3f} [{lo:.3f}, {hi:.3f}] ms, kernels {ksum:.3f} ms")
            for k, (ms, launches) in sorted(kern.items(), key=lambda kv: -kv[1][0]):
                emit(f"    {k:<28} {ms:9.3f} ms  {launches:3d} launch(es)")
        # baseline 1: the transforms of the reference's round 3 alone, device resident
        t_in = torch.from_numpy(el(4 * n, 9).view(np.int64)).cuda()
        t_out = torch.empty_like(t_in)

        def transforms_only():
            for _ in range(16):
                fft.ntt_device(F, t_in, t_out, lg + 2, offset=k1)
            fft.ntt_device(F, t_out, t_in, lg + 2, inverse=True, offset=k1)
        med, lo, hi, kern = timed(transforms_only, args.reps)
        ksum = sum(ms for ms, _ in kern.values())
        emit(f"baseline, 16 coset evaluations + 1 inverse on 4n (lw_hip_ntt_device): wall {med:.3f} [{lo:.3f}, {hi:.3f}] ms, kernels {ksum:.3f} ms")
        emit(f"round 3 / transforms-only baseline: wall {results['round 3'][0] / med:.3f}, kernels {results['round 3'][1] / ksum:.3f}")
        del t_in, t_out
        # baseline 2: the same transforms through the host-buffer entry points (17 evaluations + 1 interpolation)
        polys = [el(n + 3, 40), el(n + 2, 41)] + [el(n, 42)] * 14 + [el(n + 1, 43)]
        evals = el(4 * n, 44)

        def host_buffers():
            for c in polys:
                fft.evaluate_offset_fft(F, c, 1, 4 * n, k1)
            fft.interpolate_offset_fft(F, evals, k1)
        med, lo, hi, _ = timed(host_buffers, args.host_reps, profile=False)
        emit(f"baseline, 17 evaluate_offset_fft + 1 interpolate_offset_fft on host buffers: wall {med:.2f} [{lo:.2f}, {hi:.2f}] ms")
        emit(f"round 3 / host-buffer baseline: wall {results['round 3'][0] / med:.4f}")
        cir.close()
        del t_w, t_abc, t_z
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
