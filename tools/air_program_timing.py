#!/usr/bin/env python3
"""AIR transition programs on the device (csrc/stark_air.hip), Stark252, trace 2^20, blow-up 4 (N = 2^22): the time of
air_transition_kernel for the two-column Fibonacci AIR (two constraints, no product) and for the permutation constraint of
the read-only-memory AIR (five columns, two constants; the table lists its ops, products and temporaries), beside
  - a device-to-device copy that moves as many bytes as the kernel must read and write: (distinct columns + constraints)
    * N * 32, half of them read and half written by the copy;
  - the time its MUL count would take at the fe_mul rate recorded in profiles/poseidon.txt.
Kernel times come from lw_hip_profile_* (HIP events around the launch), after a warm-up call, as medians over --reps calls;
the copy is timed with HIP events in the same process, interleaved with the kernel calls.
usage: air_program_timing.py [--reps K] [--log2-trace L] [--out FILE]"""
import argparse
import os
import re
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from lambda_elliptic_curves_amd import _lib, fft, stark  # noqa: E402
from tools import inputs  # noqa: E402


def fe_mul_rate():
    """Gmul/s recorded in profiles/poseidon.txt, or None"""
    try:
        m = re.search(r"FE_MUL\s+([0-9.]+)\s+Gmul/s", open(os.path.join(ROOT, "profiles", "poseidon.txt")).read())
        return float(m.group(1)) if m else None
    except OSError:
        return None


def airs():
    """name -> (expressions, columns, constants)"""
    c, k = stark.cell, stark.const
    z, alpha = k(0), k(1)
    return {
        "fibonacci, 2 columns": ([c(0, 1) - c(1), c(1, 1) - c(0) - c(1)], 2, 0),
        "read-only memory, permutation": ([(z - (c(2, 1) + alpha * c(3, 1))) * c(4, 1) - (z - (c(0, 1) + alpha * c(1, 1))) * c(4)], 5, 2),
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--log2-trace", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    F = fft.Stark252PrimeField
    lg, log2_blowup = args.log2_trace, 2
    N = 1 << (lg + log2_blowup)
    rate = fe_mul_rate()
    emit(f"# {torch.cuda.get_device_name(0)}, Stark252, trace 2^{lg}, blow-up 4, N = 2^{lg + log2_blowup}, reps = {args.reps}: median [min .. max] ms")
    emit("# fe_mul rate: " + (f"{rate:.1f} Gmul/s (profiles/poseidon.txt)" if rate else "not recorded"))
    emit(f"{'AIR':<32} {'ops':>4} {'MUL':>4} {'tmps':>4} {'MiB':>8} {'kernel ms':>10} {'[min .. max]':>19} {'copy ms':>8} {'kernel/copy':>11} {'MUL ms':>8} {'kernel/MUL':>10}")
    for name, (exprs, n_cols, n_consts) in airs().items():
        program = stark.compile_transitions(exprs)
        T = program.n_transitions
        t_cols = [torch.from_numpy(inputs.rand_elems("stark252", N, 40 + c).view(np.int64)).cuda() for c in range(n_cols)]
        consts = inputs.rand_elems("stark252", n_consts, 7) if n_consts else None
        t_out = torch.empty((T, N, 4), dtype=torch.int64, device="cuda")
        nbytes = (n_cols + T) * N * 32
        t_src = torch.empty(nbytes // 2 // 8, dtype=torch.int64, device="cuda")
        t_dst = torch.empty_like(t_src)
        run = lambda: stark.transition_evaluations_device(F, program, consts, t_cols, lg, log2_blowup, t_out=t_out)
        run()
        t_dst.copy_(t_src)
        torch.cuda.synchronize()
        kernel, copy = [], []
        for _ in range(args.reps):
            _lib.profile_begin()
            run()
            torch.cuda.synchronize()
            kernel.append(sum(ms for k, (_n, ms) in _lib.profile_end().items() if k == "air_transition_kernel"))
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            t_dst.copy_(t_src)
            e1.record()
            torch.cuda.synchronize()
            copy.append(e0.elapsed_time(e1))
        km, cm = statistics.median(kernel), statistics.median(copy)
        mul_ms = program.n_mul * N / rate / 1e6 if rate and program.n_mul else None
        emit(f"{name:<32} {len(program):>4} {program.n_mul:>4} {program.n_tmps:>4} {nbytes / 2**20:8.1f} {km:10.3f} "
             f"{'[%.3f .. %.3f]' % (min(kernel), max(kernel)):>19} {cm:8.3f} {km / cm:11.2f} "
             f"{('%8.3f' % mul_ms) if mul_ms else '       -'} {('%10.2f' % (km / mul_ms)) if mul_ms else '         -'}")
        del t_cols, t_out, t_src, t_dst
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
