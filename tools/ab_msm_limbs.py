#!/usr/bin/env python3
"""Device-resident MSM time by scalar width (lw_hip_msm_limbs_device, 1 .. 8 u64 limbs) on DISTINCT points (tools/synth.py,
as bench.py builds them), widths alternated inside one process, median and spread of the repetitions.

  --table   BLS12-381 G1 and BN254 G1, L in {1, 2, 4, 6, 8} at 2^20, 2^22, 2^24 (default window rule), plus L = 4 through the
            old entry point lw_hip_msm_device: the 256-bit path against lw_hip_msm_limbs_device(..., 4, ...)
  --sweep   BLS12-381 G1, the window width c (LW_HIP_MSM_C, read per call; sets LW_HIP_TUNING=1, without which the library
            ignores it) for L in {1, 2, 6} at 2^18 .. 2^24
usage: ab_msm_limbs.py [--table] [--sweep] [--reps K] [--out FILE]"""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from lambda_elliptic_curves_amd import _lib, msm  # noqa: E402
from tools.synth import distinct_points  # noqa: E402

SWEEP = {1: (11, 13, 16, 18, 19, 20), 2: (13, 16, 17, 19, 20), 6: (16, 17, 18, 19, 20)}


def windows(bits, c):
    return 1 + bits // c


def rand_scalars(n, limbs, seed):
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    return torch.randint(-(1 << 63), (1 << 63) - 1, (n, limbs), dtype=torch.int64, device="cuda", generator=g)


def call(crv, ts, tp, n, limbs, old_entry=False):
    out = np.zeros(crv.point_words, dtype=np.uint64)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    L = _lib.lib()
    t0 = time.perf_counter()
    if old_entry:
        rc = L.lw_hip_msm_device(crv.curve, C.c_void_p(ts.data_ptr()), C.c_void_p(tp.data_ptr()), n, out.ctypes.data_as(C.c_void_p), stream)
    else:
        rc = L.lw_hip_msm_limbs_device(crv.curve, C.c_void_p(ts.data_ptr()), limbs, C.c_void_p(tp.data_ptr()), n,
                                       out.ctypes.data_as(C.c_void_p), stream)
    dt = (time.perf_counter() - t0) * 1e3   # the call returns the point to the host: it has synchronised
    assert rc == 0, _lib.last_error()
    return dt, out


def fmt(ts):
    med = statistics.median(ts)
    return "%8.2f ms  (min %.2f max %.2f, spread %.1f %%)" % (med, min(ts), max(ts), 100 * (max(ts) - min(ts)) / med)


def table(reps, emit):
    emit("## default window rule, device-resident, distinct points; median of %d alternated repetitions" % reps)
    for crv in (msm.BLS12381Curve, msm.BN254Curve):
        for lg in (20, 22, 24):
            n = 1 << lg
            tp = distinct_points(crv, n)
            scal = {L: rand_scalars(n, L, 100 * lg + L) for L in (1, 2, 4, 6, 8)}
            legs = [(L, False) for L in (1, 2, 4, 6, 8)] + [(4, True)]
            times = {k: [] for k in legs}
            outs = {}
            for leg in legs:   # warm-up (workspace, code objects)
                outs[leg] = call(crv, scal[leg[0]], tp, n, leg[0], leg[1])[1]
            assert outs[(4, True)].tobytes() == outs[(4, False)].tobytes(), "L = 4: the two entry points differ"
            for _ in range(reps):
                for leg in legs:
                    times[leg].append(call(crv, scal[leg[0]], tp, n, leg[0], leg[1])[0])
            base = statistics.median(times[(4, False)])
            for leg in legs:
                L, old = leg
                name = "L=4 lw_hip_msm_device (old entry)" if old else "L=%d lw_hip_msm_limbs_device" % L
                emit("%-20s 2^%d  %-36s %s  x%.2f of L=4" % (crv.name, lg, name, fmt(times[leg]), statistics.median(times[leg]) / base))
            del tp, scal
            torch.cuda.empty_cache()


def sweep(reps, emit):
    emit("## window sweep (LW_HIP_MSM_C), BLS12-381 G1, device-resident, distinct points; median of %d alternated repetitions" % reps)
    crv = msm.BLS12381Curve
    for lg in (18, 20, 22, 24):
        n = 1 << lg
        tp = distinct_points(crv, n)
        for L, cs in SWEEP.items():
            ts = rand_scalars(n, L, 7 * lg + L)
            times = {c: [] for c in cs}
            ref = None
            for c in cs:   # warm-up, and every c must give the same point
                os.environ["LW_HIP_MSM_C"] = str(c)
                out = call(crv, ts, tp, n, L)[1]
                ref = out if ref is None else ref
                assert out.tobytes() == ref.tobytes(), "c = %d gives another point" % c
            for _ in range(reps):
                for c in cs:
                    os.environ["LW_HIP_MSM_C"] = str(c)
                    times[c].append(call(crv, ts, tp, n, L)[0])
            os.environ.pop("LW_HIP_MSM_C", None)
            auto = [call(crv, ts, tp, n, L)[0] for _ in range(reps)]
            best = min(cs, key=lambda c: statistics.median(times[c]))
            for c in cs:
                B = 64 * L
                emit("2^%d L=%d c=%2d W=%2d top=%2d bits%s  %s%s" % (lg, L, c, windows(B, c), B - (windows(B, c) - 1) * c,
                                                                    " (split)" if B % c == 0 else "        ", fmt(times[c]),
                                                                    "  <- best" if c == best else ""))
            emit("2^%d L=%d default rule                      %s" % (lg, L, fmt(auto)))
            del ts
        del tp
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--table", action="store_true")
    ap.add_argument("--sweep", action="store_true")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.sweep:
        os.environ["LW_HIP_TUNING"] = "1"   # read once, when the library first asks for a tuning switch
    f = open(a.out, "a") if a.out else None

    def emit(line):
        print(line, flush=True)
        if f:
            f.write(line + "\n")
            f.flush()

    emit("# %s  %s" % (torch.cuda.get_device_name(0), time.strftime("%Y-%m-%d %H:%M")))
    if a.sweep:
        sweep(a.reps, emit)
    if a.table:
        table(a.reps, emit)


if __name__ == "__main__":
    main()
