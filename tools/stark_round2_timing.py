#!/usr/bin/env python3
"""STARK round 2 on the device, Stark252: summed kernel times of the batch inversion, the constraint kernel, the parts
(interpolation, split, LDE of the parts) and the paired-row commitment, each beside its compulsory bytes.
Shape: n = 2^18 and 2^20, blow-up 4, 4 columns, 4 transitions (period 1, one end exemption), 4 boundary constraints on 2
distinct steps, P = 2.  Kernel times come from lw_hip_profile_* (HIP events around every launch), after a warm-up call, as
medians over --reps calls; min and max show the spread of the box.
Compulsory bytes: constraint kernel (n_cols + n_transitions + 1) * N * 32; batch inverse 2 * n * 32.  For the batch
inverse the time 3 products per element would take at the fe_mul rate of profiles/poseidon.txt is listed beside it.
usage: stark_round2_timing.py [--reps K] [--out FILE]"""
import argparse
import os
import re
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from lambda_elliptic_curves_amd import _lib, fft, merkle, poly, stark  # noqa: E402


def rand_stark(shape, seed):
    """canonical Stark252 elements (< 2^250 < p) on the device, (*shape, 4) int64"""
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    t = torch.randint(-(1 << 63), (1 << 63) - 1, tuple(shape) + (4,), dtype=torch.int64, device="cuda", generator=g)
    t[..., 0] &= (1 << 58) - 1
    return t


def profiled(fn, reps, names=None):
    """-> [summed kernel ms per call] over the kernels in names (None: every kernel of the call)"""
    fn()
    torch.cuda.synchronize()
    totals = []
    for _ in range(reps):
        _lib.profile_begin()
        fn()
        torch.cuda.synchronize()
        prof = _lib.profile_end()
        totals.append(sum(ms for k, (_n, ms) in prof.items() if names is None or k in names))
    return totals


def fe_mul_rate():
    """Gmul/s recorded in profiles/poseidon.txt, or None"""
    try:
        m = re.search(r"FE_MUL\s+([0-9.]+)\s+Gmul/s", open(os.path.join(ROOT, "profiles", "poseidon.txt")).read())
        return float(m.group(1)) if m else None
    except OSError:
        return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=None)
    ap.add_argument("--log2-trace", type=int, nargs="*", default=[18, 20])
    args = ap.parse_args()
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    F = fft.Stark252PrimeField
    el = lambda *w: np.array(w, np.uint64)
    off = el(0x1, 0x2345, 0x6789a, 0xbcdef1)
    rate = fe_mul_rate()
    emit(f"# {torch.cuda.get_device_name(0)}, Stark252, reps = {args.reps}: median [min .. max] of the summed kernel time per call")
    emit("# blow-up 4, 4 columns, 4 transitions, 4 boundary constraints on 2 steps, P = 2; GB/s over the compulsory bytes")
    emit(f"{'step':<22} {'log2 n':>6} {'elements':>10} {'ms':>9} {'[min .. max]':>21} {'MiB':>9} {'GB/s':>8}  note")

    def row(step, lg, elems, t, nbytes, note=""):
        m = statistics.median(t)
        emit(f"{step:<22} {lg:>6} {elems:>10} {m:9.3f} {'[%.3f .. %.3f]' % (min(t), max(t)):>21} {nbytes / 2**20:9.1f} {nbytes / m / 1e6:8.0f}  {note}")

    for lg in args.log2_trace:
        n, log2_blowup, n_cols, n_tr, P = 1 << lg, 2, 4, 4, 2
        N, log2_lde = n << log2_blowup, lg + log2_blowup
        # batch inverse of n elements
        t_a = rand_stark((n,), 10 + lg)
        t_a[:, 3] |= 1
        t_b = torch.empty_like(t_a)
        t = profiled(lambda: poly.batch_inverse_device(F, t_a, n, t_b), args.reps, ("field_batch_inverse_kernel",))
        note = f"3 products per element at {rate:.1f} Gmul/s: {3 * n / rate / 1e6:.3f} ms" if rate else "fe_mul rate not recorded"
        row("batch inverse", lg, n, t, 2 * n * 32, note)
        del t_a, t_b
        # constraint evaluations
        t_cols = rand_stark((n_cols, N), 20 + lg)
        t_tev = rand_stark((n_tr, N), 30 + lg)
        t_out = torch.empty((N, 4), dtype=torch.int64, device="cuda")
        boundary = [(0, 0, el(0, 0, 0, 5), el(0, 1, 2, 3)), (1, 0, el(0, 0, 0, 6), el(0, 4, 5, 6)),
                    (2, n - 1, el(0, 0, 0, 7), el(0, 7, 8, 9)), (3, n - 1, el(0, 0, 0, 8), el(0, 10, 11, 12))]
        transitions = [dict(period=1, end_exemptions=1, coeff=el(0, 13 + k, 14, 15)) for k in range(n_tr)]
        cols = [t_cols[c] for c in range(n_cols)]
        fn = lambda: stark.constraint_evaluations_device(F, cols, lg, log2_blowup, off, boundary, transitions, t_tev, t_out=t_out)
        row("constraint kernel", lg, N, profiled(fn, args.reps, ("r2_constraint_kernel",)), (n_cols + n_tr + 1) * N * 32)
        row("  tables (x, cycles)", lg, N, profiled(fn, args.reps, ("r2_xtable_kernel", "r2_cycle_kernel", "field_batch_inverse_kernel")), 0)
        del t_cols, t_tev
        # parts: interpolation, split, LDE of the parts
        parts = {}

        def run_parts():
            parts["c"], _lens, parts["lde"] = stark.composition_parts_device(F, t_out, log2_lde, off, P, lens=False)

        row("parts", lg, N, profiled(run_parts, args.reps), (1 + 2 * P) * N * 32, "every kernel of the call; bytes: H in, parts' LDE out, parts in and out")
        # commitment
        t_nodes = torch.empty((N - 1) * 4, dtype=torch.int64, device="cuda")
        t_lde = parts["lde"]
        row("commitment", lg, N, profiled(lambda: merkle.commit_composition_device(F, t_lde, P, log2_lde, t_nodes), args.reps),
            (P * N + N - 1) * 32, "every kernel of the call")
        del t_out, t_nodes, t_lde, parts
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
