"""Which BabyBear transform sizes reach which instantiation of bb_pass_kernel (csrc/ntt_bb.hip), derived on the host from
the planner, the schedule and the predicate that picks a compiled tile shape (plan_passes, schedule_passes and bb_tile_rx
in csrc/ntt_plan.h, plain C++): a small driver is compiled with g++ and prints, for lgV in {0, 2}, L in 1..20, skip in
0..7 and aliased in {0, 1}, one line

    `bb lgV L skip aliased npass`, then per pass that runs ` | first last src r rx`

(src as PassBuf, rx = 0 for the kernel that takes its tile shape from the parameters, else 6, 7 or 8).

An instantiation is (LAST, reads the caller's words, writes the caller's words, RX, lgV): the template arguments of
bb_pass_kernel<LAST, IN64, OUT64, RX, VX> for the u64 word shapes (IN64 = reads the caller's words, OUT64 = writes them;
with u32 words both are false), with the run-time lgV of the RX = 0 kernel kept apart as well.  The test derives every
instantiation a transform of at most 2^20 memory words can reach and asserts that the size table of
tests/test_gpu_ntt_babybear_edges.py (tests/ntt_bb_cases.py) reaches each of them.

skip goes beyond the 0..3 of common blow-ups because a single pass with the tile shape compiled in exists only there:
at most 8 stages over a full tile of 2^13 words is a low-degree extension with blow-up 32 and more (the extension: 8).

A compiled middle pass of 8 stages needs 2^23 words and more (three passes with 8 stages in the second are 23 stages at
the least, the split being even): out of reach of a test of a few seconds, it is left to test_max_size_2_24_roundtrip_u32."""
import os
import subprocess
import textwrap

from tests import ntt_bb_cases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

DRIVER = r"""
#include <cstdio>
#include "%s/lambda_elliptic_curves_amd/csrc/ntt_plan.h"
using namespace lw;
int main() {
    for (uint32_t lgV = 0; lgV <= 2; lgV += 2)
        for (uint32_t L = 1; L <= 20; L++)
            for (uint32_t skip = 0; skip <= 7 && skip < L; skip++)
                for (int aliased = 0; aliased < 2; aliased++) {
                    const NttPlan pl = plan_passes(L + lgV, L, skip, BB_TILE_LOG, BB_KMAX, false);   // as bb_run does
                    const PassSchedule sc = schedule_passes(pl, false, aliased != 0);
                    printf("bb %%u %%u %%u %%d %%d", lgV, L, skip, aliased, sc.npass);
                    for (int q = 0; q < sc.npass; q++) {
                        const PassStep &st = sc.step[q];
                        printf(" | %%d %%d %%d %%u %%u", (int)st.first, (int)st.last, (int)st.src, st.r, bb_tile_rx(st, lgV));
                    }
                    printf("\n");
                }
    return 0;
}
"""

IN, STAGED, WORK, OUT = range(4)   # PassBuf
_lines_of = {}


def _passes(tmp_path):
    """(lgV, L, skip, aliased) -> [(first, last, src, r, rx)] per pass; compiled and run once per session"""
    if "bb" not in _lines_of:
        src = tmp_path / "bb_shapes.cpp"
        src.write_text(textwrap.dedent(DRIVER % ROOT))
        exe = tmp_path / "bb_shapes"
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                               "-fno-sanitize-recover=all", "-o", str(exe), str(src)])
        out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
        assert out.returncode == 0, out.stderr[-2000:]
        table = {}
        for line in out.stdout.splitlines():
            head, *passes = line.split(" | ")
            tag, lgV, L, skip, aliased, npass = head.split()
            assert tag == "bb" and len(passes) == int(npass), line
            table[(int(lgV), int(L), int(skip), int(aliased))] = [tuple(int(v) for v in p.split()) for p in passes]
        _lines_of["bb"] = table
    return _lines_of["bb"]


def _instantiations(passes, lgV):
    return {(last, int(src != WORK), last, rx, lgV) for first, last, src, r, rx in passes}


def _reached_by(table, entries):
    """the instantiations the entries of a size table reach: a plain transform runs out of place and in place, a
    low-degree extension out of place only"""
    got = set()
    for lgV, L, skip in entries:
        for aliased in ((0, 1) if skip == 0 else (0,)):
            got |= _instantiations(table[(lgV, L, skip, aliased)], lgV)
    return got


def _reachable(table):
    got = set()
    for (lgV, L, skip, aliased), passes in table.items():
        if L + lgV <= cases.MAX_LOG_WORDS and not (skip and aliased):
            got |= _instantiations(passes, lgV)
    return got


def test_driver_covers_the_inputs_and_the_schedule_is_the_one_the_kernel_selection_assumes(tmp_path):
    table = _passes(tmp_path)
    assert set(table) == {(v, L, s, a) for v in (0, 2) for L in range(1, 21) for s in range(0, min(8, L)) for a in (0, 1)}
    for (lgV, L, skip, aliased), passes in table.items():
        key = (lgV, L, skip, aliased)
        assert sum(r for _, _, _, r, _ in passes) == L - skip, key
        assert [p[0] for p in passes] == [1] + [0] * (len(passes) - 1), key
        assert [p[1] for p in passes] == [0] * (len(passes) - 1) + [1], key
        # only the first pass reads the caller's words (or their staged copy), only the last writes them
        assert [p[2] for p in passes] == [STAGED if len(passes) == 1 and aliased else IN] + [WORK] * (len(passes) - 1), key
        for first, last, src, r, rx in passes:
            assert rx in (0, r) and rx in (0, 6, 7, 8), key
        # aliasing changes buffers, never the kernel
        assert [p[3:] for p in passes] == [p[3:] for p in table[(lgV, L, skip, 0)]], key


def test_size_table_reaches_every_reachable_instantiation(tmp_path):
    table = _passes(tmp_path)
    assert all(L + lgV <= cases.MAX_LOG_WORDS and 0 <= skip < L for lgV, L, skip in cases.SIZES)
    assert len(set(cases.SIZES)) == len(cases.SIZES)
    reachable = _reachable(table)
    print("reachable instantiations (LAST, reads caller's words, writes caller's words, RX, lgV) and the table entries that reach them:")
    for inst in sorted(reachable):
        by = [e for e in cases.SIZES if inst in _reached_by(table, [e])]
        print("  ", inst, by)
    missing = reachable - _reached_by(table, cases.SIZES)
    assert not missing, sorted(missing)
    # every compiled shape, in both positions it can take below 2^20 words and as a last pass, is among them
    for lgV in (0, 2):
        for rx in (6, 7, 8):
            assert (0, 1, 0, rx, lgV) in reachable and (1, 0, 1, rx, lgV) in reachable
    assert {rx for last, rc, wc, rx, lgV in reachable if not last and not rc and lgV == 0} == {0, 7}
    assert {rx for last, rc, wc, rx, lgV in reachable if not last and not rc and lgV == 2} == {6}


def test_every_entry_of_the_size_table_is_as_its_comment_says(tmp_path):
    table = _passes(tmp_path)
    plan = lambda lgV, L, skip: [(r, rx) for _, _, _, r, rx in table[(lgV, L, skip, 0)]]
    want = {
        (0, 8, 0): [(8, 0)], (0, 12, 0): [(6, 0), (6, 0)], (0, 13, 0): [(7, 7), (6, 6)], (0, 15, 0): [(8, 8), (7, 7)],
        (0, 16, 0): [(8, 8), (8, 8)], (0, 17, 0): [(6, 6), (6, 0), (5, 0)], (0, 18, 0): [(6, 6), (6, 0), (6, 6)],
        (0, 20, 0): [(7, 7), (7, 7), (6, 6)], (0, 16, 1): [(8, 8), (7, 7)], (0, 15, 3): [(6, 0), (6, 6)],
        (0, 18, 2): [(8, 8), (8, 8)], (2, 11, 0): [(6, 6), (5, 0)], (2, 13, 0): [(7, 7), (6, 6)], (2, 15, 0): [(8, 8), (7, 7)],
        (2, 16, 0): [(8, 8), (8, 8)], (2, 17, 0): [(6, 6), (6, 6), (5, 0)], (2, 18, 0): [(6, 6), (6, 6), (6, 6)],
        (2, 13, 2): [(6, 6), (5, 0)], (0, 13, 5): [(8, 8)], (0, 13, 6): [(7, 7)], (0, 13, 7): [(6, 6)], (2, 5, 0): [(5, 0)],
        (2, 9, 0): [(5, 0), (4, 0)], (2, 11, 3): [(8, 8)], (2, 11, 4): [(7, 7)], (2, 11, 5): [(6, 6)],
    }
    assert set(want) == set(cases.SIZES)
    for key, rows in want.items():
        assert plan(*key) == rows, key


def test_the_two_thresholds_the_gpu_test_relies_on(tmp_path):
    table = _passes(tmp_path)
    compiled = lambda lgV, L, skip: any(rx for _, _, _, _, rx in table[(lgV, L, skip, 0)])
    # L = 12 is the largest base-field size with no compiled shape, whatever the blow-up
    assert not any(compiled(0, L, s) for L in range(1, 13) for s in range(0, min(8, L)))
    assert all(compiled(0, L, 0) for L in range(13, 21))
    # the first compiled middle pass (work buffer to work buffer): L = 20 for the base field, L = 17 for the extension
    def middle(lgV, L):
        return any(rx for s in range(0, min(8, L)) for first, last, src, r, rx in table[(lgV, L, s, 0)] if not first and not last)
    assert [L for L in range(1, 21) if middle(0, L)] == [20]
    assert [L for L in range(1, 19) if middle(2, L)] == [17, 18]


def test_a_size_that_alone_reaches_an_instantiation_cannot_leave_the_table(tmp_path):
    """without (0, 20, 0) nothing runs the base field's compiled middle pass, without (2, 17, 0) and (2, 18, 0) nothing the
    extension's, without (0, 13, 5) nothing a single pass of 8 stages with the tile shape compiled in"""
    table = _passes(tmp_path)
    reachable = _reachable(table)
    for gone, inst in (([(0, 20, 0)], (0, 0, 0, 7, 0)), ([(2, 17, 0), (2, 18, 0)], (0, 0, 0, 6, 2)), ([(0, 8, 0)], (1, 1, 1, 0, 0)),
                       ([(0, 13, 5)], (1, 1, 1, 8, 0)), ([(2, 9, 0)], (0, 1, 0, 0, 2))):
        rest = [e for e in cases.SIZES if e not in gone]
        assert reachable - _reached_by(table, rest) == {inst}, gone
