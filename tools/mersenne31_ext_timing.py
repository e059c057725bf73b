#!/usr/bin/env python3
"""The Mersenne31 quartic extension on the device (csrc/mersenne31_ext.hip), every step next to its BabyBear Fp4 counterpart
at the shapes of tools/babybear_ext_timing.py and next to a device copy of the bytes it moves, all timed in one process.
  pointwise  mul and inv over 2^24 elements
  evaluate   8 columns of 2^20 coefficients at 3 points (the call waits for its values)
  deep       8 columns of 2^22 rows, 3 points
  layer      2^21 values -> 2^20, Monolith tree with 2^19 leaves, against its parts called one by one: the fold alone and
             monolith.commit_columns_device over eight columns of 2^19 words; the BabyBear layer 2^20 -> 2^19 on 2^21 beside it
  kernels    device time of every kernel of one call of each (lw_hip_profile_begin / end), after the timed runs
usage: mersenne31_ext_timing.py [--out FILE]"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools import babybear_ext_timing as B  # noqa: E402

LOG_POINTWISE, LOG_COEFFS, LOG_DOMAIN, COLUMNS, POINTS, LOG_LAYER, ROUNDS = B.LOG_POINTWISE, B.LOG_COEFFS, B.LOG_DOMAIN, B.COLUMNS, B.POINTS, 21, 5
P = (1 << 31) - 1


def words(count, seed):
    """words below p, from the BabyBear inputs of tools/inputs.py (its p is below 2^31 - 1)"""
    return B.words(count, seed)


def circle_point(t):
    """a point of the circle over QM31 from a parameter, in plain integers: ((1 - t^2) / (1 + t^2), 2t / (1 + t^2))"""
    def cmul(a, b):
        return ((a[0] * b[0] - a[1] * b[1]) % P, (a[0] * b[1] + a[1] * b[0]) % P)

    def mul(a, b):
        p0, p1 = cmul(a[:2], b[:2]), cmul(a[2:], b[2:])
        cr = cmul(((a[0] + a[2]) % P, (a[1] + a[3]) % P), ((b[0] + b[2]) % P, (b[1] + b[3]) % P))
        return ((p0[0] + 2 * p1[0] - p1[1]) % P, (p0[1] + 2 * p1[1] + p1[0]) % P, (cr[0] - p0[0] - p1[0]) % P, (cr[1] - p0[1] - p1[1]) % P)

    def inv(a):
        s, t2 = cmul(a[:2], a[:2]), cmul(a[2:], a[2:])
        n = ((s[0] - 2 * t2[0] + t2[1]) % P, (s[1] - 2 * t2[1] - t2[0]) % P)
        ni = pow((n[0] * n[0] + n[1] * n[1]) % P, P - 2, P)
        c = (n[0] * ni % P, -n[1] * ni % P)
        return cmul(a[:2], c) + cmul((-a[2] % P, -a[3] % P), c)
    t2 = mul(t, t)
    d = inv(((1 + t2[0]) % P,) + t2[1:])
    return mul(((1 - t2[0]) % P, -t2[1] % P, -t2[2] % P, -t2[3] % P), d), mul(tuple(2 * x % P for x in t), d)


def both(label, shape, t_m31, t_bb4, moved_words):
    c = B.timed(B.copy_of(moved_words))
    B.report("m31 " + label, shape, t_m31, c, moved_words)
    B.report("bb4 " + label, shape, t_bb4, c, moved_words)
    print(f"RESULT {'m31 / bb4':<16} {label:<12} {t_m31[0] / t_bb4[0]:.2f}")


def run():
    import numpy as np
    import torch
    from lambda_elliptic_curves_amd import _lib, monolith
    from lambda_elliptic_curves_amd import babybear_ext as BB
    from lambda_elliptic_curves_amd import mersenne31_ext as E
    from lambda_elliptic_curves_amd.errors import check
    from tools import inputs
    n, rows, big, layer_n = 1 << LOG_COEFFS, 1 << LOG_DOMAIN, 1 << LOG_POINTWISE, 1 << LOG_LAYER
    bb_pts = B.points(POINTS, 5)
    pts = [circle_point(t) for t in B.points(POINTS, 6)]
    h = int(inputs.offset_elem("babybear_u32", 7)[0])
    tab = [B.points(POINTS, 20 + k) for k in range(COLUMNS)]
    # pointwise
    t_a, t_b, t_out = words(4 * big, 1), words(4 * big, 2), torch.empty(4 * big, dtype=torch.int32, device="cuda")
    for label, m_op, b_op, moved in (("mul", E.MUL, BB.MUL, 12 * big), ("inv", E.INV, BB.INV, 8 * big)):
        both(label, f"2^{LOG_POINTWISE} elements", B.timed(lambda: E.pointwise_device(m_op, t_a, t_b, t_out, big)),
             B.timed(lambda: BB.pointwise_device(b_op, t_a, t_b, t_out, big)), moved)
    # evaluate
    t_cols = words(COLUMNS * rows, 3)
    both("evaluate", f"{COLUMNS} x 2^{LOG_COEFFS}, {POINTS} points", B.timed(lambda: E.evaluate_device(t_cols, COLUMNS, LOG_COEFFS, pts)),
         B.timed(lambda: BB.evaluate_device(t_cols, COLUMNS, n, bb_pts)), COLUMNS * n)
    # DEEP
    t_deep = torch.empty(4 * rows, dtype=torch.int32, device="cuda")
    both("deep", f"{COLUMNS} x 2^{LOG_DOMAIN}, {POINTS} points", B.timed(lambda: E.deep_quotients_device(t_cols, COLUMNS, LOG_DOMAIN, pts, tab, tab, t_deep)),
         B.timed(lambda: BB.deep_quotients_device(t_cols, COLUMNS, LOG_DOMAIN, bb_pts, tab, tab, t_deep, offset=h)), (COLUMNS + 4) * rows)
    # layer: the call, the fold alone, the tree alone
    t_v = words(4 * layer_n, 8)
    half = layer_n // 2
    t_folded, t_pairs = torch.empty(4 * half, dtype=torch.int32, device="cuda"), torch.empty(4 * half, dtype=torch.int32, device="cuda")
    t_nodes = torch.empty((half - 1, 8), dtype=torch.int32, device="cuda")
    zeta, root = np.array(B.points(1, 12)[0], np.uint32), np.zeros(8, np.uint32)
    lib, L = _lib.lib(), _lib

    def layer():
        check(lib.lw_mersenne31_ext4_fri_layer_device(L.device_ptr(t_v), 0, LOG_LAYER, L.host_ptr(zeta), 0, L.device_ptr(t_folded), 0, ROUNDS,
                                                        L.device_ptr(t_pairs), L.device_ptr(t_nodes), L.host_ptr(root), L.stream_ptr(None)))

    fold = lambda: E.fri_fold_device(t_v, LOG_LAYER, zeta, False, t_folded)
    commit = lambda: monolith.commit_columns_device(ROUNDS, t_pairs, 8, LOG_LAYER - 2, t_nodes, bit_reverse=False)
    tl, tf, tc = B.timed(layer), B.timed(fold), B.timed(commit)
    parts = tf[0] + tc[0]
    shape = f"2^{LOG_LAYER} -> 2^{LOG_LAYER - 1}"
    print(f"RESULT m31 layer    {shape:<28} {B.fmt(tl)}   parts: fold {B.fmt(tf)} + monolith commit 8 columns {B.fmt(tc)} = {parts:8.4f} ms"
          f"   layer / parts = {tl[0] / parts:.3f}   tree / layer = {tc[0] / tl[0]:.2f}")
    B.report("m31 fold", shape, tf, B.timed(B.copy_of(6 * layer_n)), 6 * layer_n)
    bb_layer, bb_fold, _, _ = B.layer_calls()
    tbl, tbf = B.timed(bb_layer), B.timed(bb_fold)
    print(f"RESULT bb4 layer    2^{LOG_COEFFS} -> 2^{LOG_COEFFS - 1} on 2^{LOG_DOMAIN - 1}       {B.fmt(tbl)}   fold alone {B.fmt(tbf)}   m31 layer / bb4 layer = {tl[0] / tbl[0]:.2f}")
    # kernels
    calls = [("pointwise mul", lambda: E.pointwise_device(E.MUL, t_a, t_b, t_out, big)), ("pointwise inv", lambda: E.pointwise_device(E.INV, t_a, None, t_out, big)),
             ("evaluate", lambda: E.evaluate_device(t_cols, COLUMNS, LOG_COEFFS, pts)),
             ("deep", lambda: E.deep_quotients_device(t_cols, COLUMNS, LOG_DOMAIN, pts, tab, tab, t_deep)), ("layer", layer)]
    for label, fn in calls:
        fn()
        torch.cuda.synchronize()
        _lib.profile_begin()
        for _ in range(B.CALLS):
            fn()
        torch.cuda.synchronize()
        for kname, (launches, ms) in sorted(_lib.profile_end().items()):
            print(f"KERNEL {label:<14} {kname:<28} {launches / B.CALLS:g} per call  {ms / launches:8.4f} ms each")


class Tee:
    def __init__(self, stream):
        self.stream, self.lines = stream, []

    def write(self, text):
        self.stream.write(text)
        self.lines.append(text)

    def flush(self):
        self.stream.flush()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mersenne31_ext.txt"))
    args = ap.parse_args()
    head = [f"# Mersenne31 quartic extension beside the BabyBear one: wall ms per call, median [min .. max] of {B.SAMPLES} samples of {B.CALLS} calls enqueued",
            "# back to back after a warm-up, stream synchronised, one process; a copy is torch's device-to-device copy of half the words the call moves",
            "# (read once, written once); the spread beside a ratio is the half range of both sides.  KERNEL lines: device time between events."]
    tee = Tee(sys.stdout)
    sys.stdout = tee
    try:
        run()
    finally:
        sys.stdout = tee.stream
        got = [ln[7:] for ln in "".join(tee.lines).splitlines() if ln.startswith(("RESULT ", "KERNEL "))]
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(head + (got or ["not measured yet"])) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
