"""The bound plan of the lazy Stark252 NTT passes (csrc/ntt_bound_plan.h) and the helpers that carry it out
(fe_sub_qp, fe_add_cp, fe_reduce_offset, fe_butterfly_raw in csrc/field.cuh), without a GPU.

A host program compiled from the two headers prints the plan for every pass length and runs the offset reduction and the
add/sub network of one radix-4 register step on operand edges; everything is compared with Python integers.

The plan's two guarantees, checked here by exact interval propagation for r = 1..8 and for both kinds of pass input
(any 256-bit value behind a lazy pass, a value below p in a first pass):
  * at every stage that subtracts without adding 2p, the minuend is at least 2p (a product is at most 2p - 1, and at most
    p on the unit-twiddle path, where it is fe_reduce_full of the operand);
  * no value reaches 2^256 anywhere in the pass, and none goes below zero.
"""
import functools
import itertools
import os
import subprocess
import tempfile
import textwrap

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "lambda_elliptic_curves_amd", "csrc")

P = 2**251 + 17 * 2**192 + 1
W = 2**256
X_EDGES = [0, P - 1, P, 2**251 - 1, 2**251, 30 * P, W - 1]
T_EDGES = [0, 2 * P - 1]
OFFSETS = [13, 15]   # the multiples the plan uses for r = 8 / 6 and for r = 7


def _limbs(v):
    return "{" + ", ".join("0x%08xu" % ((v >> (32 * i)) & 0xffffffff) for i in range(8)) + "}"


@functools.lru_cache(maxsize=None)
def _host_output():
    """stdout of the host program as a list of token lists"""
    src = textwrap.dedent("""
        #include <cstdio>
        struct uint4 { unsigned x, y, z, w; };
        static inline uint4 make_uint4(unsigned a, unsigned b, unsigned c, unsigned d) { return uint4{a, b, c, d}; }
        #include "field.cuh"
        #include "ntt_bound_plan.h"
        using namespace lw;
        typedef Fe<Stark252> E;
        static const unsigned XE[%(nx)d][8] = {%(xe)s};
        static const unsigned TE[%(nt)d][8] = {%(te)s};
        static E mk(const unsigned *w) { E r; for (int i = 0; i < 8; i++) r.v[i] = w[i]; return r; }
        static void put(const E &a) { for (int i = 7; i >= 0; i--) printf("%%08x", a.v[i]); }
        template <int C> static void reductions() {
            for (int i = 0; i < %(nx)d; i++) {
                printf("red %%d %%d ", C, i); put(fe_reduce_offset<C>(mk(XE[i]))); printf("\\n");
                printf("add %%d %%d ", C, i); put(fe_add_cp<C>(mk(XE[i]))); printf("\\n");
            }
        }
        // the add/sub network of one radix-4 register step as ntt_butterflies walks it (K = 2), products given
        template <bool FREE> static void step(int i0, int i1, int tm) {
            E x[4] = {fe_reduce_offset<13>(mk(XE[i0])), fe_reduce_offset<13>(mk(XE[i1])), mk(TE[tm & 1]), mk(TE[(tm >> 1) & 1])};
            fe_butterfly_raw<Stark252, FREE>(x[0], x[2]);   // stage 0
            fe_butterfly_raw<Stark252, FREE>(x[1], x[3]);
            printf("step %%d %%d %%d %%d", (int)FREE, i0, i1, tm);
            for (int j = 0; j < 4; j++) { printf(" "); put(x[j]); }
            E t1 = mk(TE[(tm >> 2) & 1]), t3 = mk(TE[(tm >> 3) & 1]);   // the products of x[1] and x[3] with the stage-1 twiddles
            x[1] = t1; x[3] = t3;
            fe_butterfly_raw<Stark252, FREE>(x[0], x[1]);   // stage 1
            fe_butterfly_raw<Stark252, FREE>(x[2], x[3]);
            for (int j = 0; j < 4; j++) { printf(" "); put(x[j]); }
            printf("\\n");
        }
        int main() {
            for (int r = 1; r <= NTT_LAZY_MAX_STAGES; r++) printf("plan %%d %%d %%d\\n", r, ntt_bound_plan(r).c, ntt_bound_plan(r).nfree);
            printf("top %%d\\n", NTT_LAZY_TOP_MULTIPLE);
            reductions<13>(); reductions<15>();
            for (int i = 0; i < %(nx)d; i++) { printf("sub %%d ", i); put(fe_sub_qp(mk(XE[i]))); printf("\\n"); }
            for (int i0 = 0; i0 < %(nx)d; i0++)
                for (int i1 = 0; i1 < %(nx)d; i1++)
                    for (int tm = 0; tm < 16; tm++) { step<true>(i0, i1, tm); step<false>(i0, i1, tm); }
            return 0;
        }
    """) % {"nx": len(X_EDGES), "nt": len(T_EDGES), "xe": ", ".join(_limbs(v) for v in X_EDGES),
            "te": ", ".join(_limbs(v) for v in T_EDGES)}
    with tempfile.TemporaryDirectory() as tmp:
        cpp, exe = os.path.join(tmp, "t.cpp"), os.path.join(tmp, "t")
        with open(cpp, "w") as f:
            f.write(src)
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-fsanitize=undefined", "-fno-sanitize-recover=all", "-I", CSRC,
                               "-o", exe, cpp])
        out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    return [ln.split() for ln in out.stdout.splitlines()]


def _plans():
    return {int(t[1]): (int(t[2]), int(t[3])) for t in _host_output() if t[0] == "plan"}


def _reduced(x):
    """x - (x >> 251) p as an integer (may be negative)"""
    return x - (x >> 251) * P


def test_reduction_difference_range():
    """d = x - (x >> 251) p over all 256-bit x, exactly: q = x >> 251 is constant on [q 2^251, (q + 1) 2^251), where d is
    increasing in x"""
    lo = min(_reduced(q << 251) for q in range(32))
    hi = max(_reduced(((q + 1) << 251) - 1) for q in range(32))
    assert -2**202 < lo and hi <= P
    assert 31 * P < W < 32 * P


def _propagate(r, c, nfree, lazy_in):
    """(lo, hi) of the values of a pass stage by stage, as exact integers.  Returns the list of (stage, free, lo before,
    lo after, hi after).  Every stage's minuends are values of the previous stage (or the offset elements on load), so one
    interval serves all of them."""
    if lazy_in:
        lo = c * P + min(_reduced(q << 251) for q in range(32))
        hi = c * P + max(_reduced(((q + 1) << 251) - 1) for q in range(32))
    else:
        lo, hi = c * P, c * P + P - 1
    tmax = 2 * P - 1   # a product; the unit-twiddle path gives at most p, inside the same bound
    rows = []
    for s in range(r):
        free = s < nfree
        before = lo
        sub_lo = lo - tmax if free else lo + 2 * P - tmax
        sub_hi = hi if free else hi + 2 * P
        lo, hi = min(lo, sub_lo), max(hi + tmax, sub_hi)
        rows.append((s, free, before, lo, hi))
    return rows


def _guarantees(r, c, nfree, lazy_in):
    rows = _propagate(r, c, nfree, lazy_in)
    free_ok = all(before >= 2 * P for _, free, before, _, _ in rows if free)
    range_ok = all(lo >= 0 and hi < W for _, _, _, lo, hi in rows)
    return free_ok, range_ok


@pytest.mark.parametrize("lazy_in", [True, False], ids=["any-256-bit-input", "input-below-p"])
@pytest.mark.parametrize("r", range(1, 9))
def test_plan_keeps_both_guarantees(r, lazy_in):
    c, nfree = _plans()[r]
    assert 1 <= c <= 15 and 0 <= nfree <= r
    assert _guarantees(r, c, nfree, lazy_in) == (True, True)


def test_plan_values():
    plans = _plans()
    assert plans[8] == (13, 6) and plans[7] == (15, 7) and plans[6] == (13, 6)
    assert all(plans[r][1] == r for r in range(1, 8))
    assert [t for t in _host_output() if t[0] == "top"] == [["top", "31"]]


def test_plan_is_tight_at_eight_stages():
    """r = 8 with seven free stages breaks one of the two guarantees whatever multiple of p is added on load, and so does
    a smaller multiple than the plan's with its six.  The input is the lazy one: free or not is compiled into a kernel, and
    every kernel also runs as a middle or last pass.  (A first pass alone would get by with 14p and seven free stages,
    2p + 6 at the bottom and 31p - 9 at the top; no kernel is built for that.)"""
    for c in range(0, 33):
        assert _guarantees(8, c, 7, True) != (True, True), c
    assert _guarantees(8, 14, 7, False) == (True, True)
    c, nfree = _plans()[8]
    assert _guarantees(8, c - 1, nfree, True) != (True, True)


def test_offset_reduction_on_edges():
    rows = _host_output()
    subs = {int(t[1]): int(t[2], 16) for t in rows if t[0] == "sub"}
    assert len(subs) == len(X_EDGES)
    for i, x in enumerate(X_EDGES):
        assert subs[i] == _reduced(x) % W, hex(x)
    seen = 0
    for t in rows:
        if t[0] not in ("red", "add"):
            continue
        c, x, got = int(t[1]), X_EDGES[int(t[2])], int(t[3], 16)
        if t[0] == "red":
            want = _reduced(x) + c * P
            assert c * P - 2**202 < want <= (c + 1) * P and want % P == x % P
        else:
            want = (x + c * P) % W
        assert got == want, (t[0], c, hex(x))
        seen += 1
    assert seen == 2 * len(OFFSETS) * len(X_EDGES)


def test_radix4_step_network_on_edges():
    """x0, x1 = the offset reduction (13p) of every pair of edges, all four products of the step at 0 or 2p - 1: limb for
    limb against integers, and in the free form no difference goes below zero"""
    rows = [t for t in _host_output() if t[0] == "step"]
    assert len(rows) == 2 * 16 * len(X_EDGES) ** 2
    for t in rows:
        free, i0, i1, tm = (int(v) for v in t[1:5])
        got = [int(v, 16) for v in t[5:13]]   # the four values after stage 0, then after stage 1
        x0, x1 = (_reduced(X_EDGES[i]) + 13 * P for i in (i0, i1))
        ta, tb, tc, td = (T_EDGES[(tm >> k) & 1] for k in range(4))
        k2p = 0 if free else 2 * P
        a0, a2, a1, a3 = x0 + ta, x0 + k2p - ta, x1 + tb, x1 + k2p - tb
        want = [a0, a1, a2, a3, a0 + tc, a0 + k2p - tc, a2 + td, a2 + k2p - td]
        assert all(0 <= v < W for v in want)
        assert got == want, t[1:5]
