// Pass planning shared by the 256-bit-field NTT (ntt256.hip), the BabyBear NTT (ntt_bb.hip) and, through tile_pass.cuh, the circle FFT
// (circle.hip) and the Goldilocks NTT (goldilocks.hip): how the stages of a transform are cut into passes, how wide each pass's tile is and how a pass is split into register steps
// (plan_passes); which buffer each pass of a plan reads and writes and in which order passes and steps run (schedule_passes, the data pass_run.h launches from); how a wide batch is cut (split_batch).
// Host only, plain C++ (no HIP header): tests/test_ntt_plan_cpu.py compiles it with g++ and pins every plan and every schedule.
#pragma once
#include <stdint.h>

namespace lw {

// stages per pass: the staged twiddles (ltw[2][256], 255 entries) and the 17p lazy bound both need r <= 8 (ntt_kernels.cuh)
constexpr uint32_t NTT_MAX_R = 8;
constexpr uint32_t MAX_BATCH = 32768;   // grid.y carries the batch: wider ones are split (split_batch)

struct NttPlan {
    int npass;
    uint32_t s0[8], r[8], logC[8];   // per pass: first stage, stages, log2 columns of the tile (in words)
    uint32_t nsteps[8], k[8][8];     // per pass: register steps and the stages of each, sum k = r
};

// Stages [skip, L) of a transform of 2^L elements whose word array has Lw index bits (Lw = L for the 256-bit fields, one
// word per element; Lw = L + lgV for BabyBear, 2^lgV components per element).  The first `skip` stages of a zero-padded
// input only replicate it (see ntt256_run) and are not planned.  A workgroup's tile holds 2^tile_log words, a register
// step runs at most kmax stages, a pass at most max_r (the diagnostic switches of the circle transform and of the
// Goldilocks NTT lower it to reach the higher pass counts at small sizes, tile_max_r in tile_pass.cuh).
inline NttPlan plan_passes(uint32_t Lw, uint32_t L, uint32_t skip, uint32_t tile_log, uint32_t kmax, bool full_last_pass,
                           uint32_t max_r = NTT_MAX_R) {
    NttPlan pl{};
    const uint32_t Ls = L - skip;
    pl.npass = (int)((Ls + max_r - 1) / max_r);
    if (pl.npass < 1) pl.npass = 1;
    // even split, the longer passes first
    uint32_t rr[8];
    uint32_t base = Ls / pl.npass, extra = Ls % pl.npass;
    for (int i = 0; i < pl.npass; i++) rr[i] = base + ((uint32_t)i < extra ? 1 : 0);
    // full_last_pass (the 256-bit fields), from 2^16 up: the last pass (per-element twiddles, bit-reversed stores,
    // wave-local exchanges) takes a full max_r stages and the others share the rest as evenly as possible in EVEN sizes —
    // an odd pass ends in a radix-2 register step with two items per thread.  Measured: 2^20 (7,7,6) 0.1056 -> (6,6,8)
    // 0.1030 ms, 2^22 (8,7,7) 0.3588 -> (6,8,8) 0.3533, 2^26 (7,7,6,6) 6.45 -> (6,6,6,8) 6.19 ms; a short LAST pass is
    // the worst choice (2^26 (8,8,8,2): 9.1 ms).
    if (full_last_pass && pl.npass >= 2 && Ls >= 16 && Ls > max_r) {
        const int q = pl.npass - 1;
        rr[q] = max_r;
        const uint32_t R = Ls - max_r;
        base = R / q;
        extra = R % q;
        for (int i = 0; i < q; i++) rr[i] = base + ((uint32_t)i >= (uint32_t)q - extra ? 1 : 0);
        for (int i = 0; i + 1 < q; i++)
            if ((rr[i] & 1) && (rr[i + 1] & 1) && rr[i + 1] < max_r && rr[i] > 1) {
                rr[i]--;
                rr[i + 1]++;
            }
    }
    uint32_t s = skip;
    for (int i = 0; i < pl.npass; i++) {
        const uint32_t r = rr[i];
        pl.s0[i] = s;
        pl.r[i] = r;
        // the tile is as wide as it has room for and the vector has columns
        const uint32_t room = tile_log - r;
        uint32_t avail = Lw - s - r;   // non-last: log2 of the row stride; last: 0 unless multi-pass
        if (i == pl.npass - 1) avail = Lw - r;
        pl.logC[i] = room < avail ? room : avail;
        // register steps: as few as kmax allows, the longer ones first
        const uint32_t nsteps = (r + kmax - 1) / kmax;
        uint32_t left = r;
        pl.nsteps[i] = nsteps;
        for (uint32_t j = 0; j < nsteps; j++) {
            const uint32_t k = (left + (nsteps - j) - 1) / (nsteps - j);
            pl.k[i][j] = k;
            left -= k;
        }
        s += r;
    }
    return pl;
}

// The passes of a transform in the order they run and the buffer each one reads and writes.  Only the first pass reads
// the caller's input, only the last writes the caller's output, everything between lies in one work buffer: a pass other
// than the plan's last (`lo`, which reorders across tiles) rewrites the words of its own tile, so it may run from the work
// buffer into the work buffer.  A single pass on aliased buffers (d_in == d_out) reads a copy in the work buffer (`stage`).
enum PassBuf { PASS_IN, PASS_STAGED, PASS_WORK, PASS_OUT };   // the caller's input, its copy in the work buffer, the work buffer, the caller's output
struct PassStep {
    int i;                          // index into the plan
    bool first, last, lo;           // the first / last pass that runs; the plan's last pass
    PassBuf src, dst;
    uint32_t s0, r, logC;           // the plan's entry
    uint32_t nsteps, k[8], t0[8];   // register steps in the order they run: stages t0 .. t0 + k - 1 of the pass
};
struct PassSchedule {
    bool stage;
    int npass;
    PassStep step[8];
};
// `backward`: the passes, and the steps of each, run in reverse order (the backward butterfly of the circle interpolation)
inline PassSchedule schedule_passes(const NttPlan &pl, bool backward, bool aliased) {
    PassSchedule sc{};
    sc.stage = pl.npass == 1 && aliased;
    sc.npass = pl.npass;
    for (int q = 0; q < pl.npass; q++) {
        PassStep &st = sc.step[q];
        const int i = st.i = backward ? pl.npass - 1 - q : q;
        st.first = q == 0;
        st.last = q == pl.npass - 1;
        st.lo = i == pl.npass - 1;
        st.src = !st.first ? PASS_WORK : sc.stage ? PASS_STAGED : PASS_IN;
        st.dst = st.last ? PASS_OUT : PASS_WORK;
        st.s0 = pl.s0[i];
        st.r = pl.r[i];
        st.logC = pl.logC[i];
        st.nsteps = pl.nsteps[i];
        uint32_t t0 = 0;
        for (uint32_t j = 0; j < st.nsteps; j++) {
            const uint32_t at = backward ? st.nsteps - 1 - j : j;
            st.k[at] = pl.k[i][j];
            st.t0[at] = t0;
            t0 += pl.k[i][j];
        }
    }
    return sc;
}

// BabyBear (ntt_bb.hip): the tile of a pass and the stages of a register step
constexpr int BB_TILE_LOG = 13;   // 8192 u32 = 32 KiB of LDS
constexpr int BB_KMAX = 4;        // radix-16 register steps

// Which bb_pass_kernel a pass of a BabyBear transform takes: 8, 7 or 6 = the kernel with a full-size tile of that many
// stages compiled in (2^(13 - r) columns x components, two register steps of 4+4, 4+3 or 3+3 stages, lgV = 0 or 2), 0 = the
// kernel that takes its tile shape from the parameters.  Here, not in ntt_bb.hip, so that
// tests/test_ntt_bb_shapes_cpu.py can tell without a device which sizes reach which instantiation.
inline uint32_t bb_tile_rx(const PassStep &st, uint32_t lgV) {
    const bool full = st.r >= 6 && st.r <= 8 && st.logC == BB_TILE_LOG - st.r && st.nsteps == 2 && st.k[0] == (st.r >= 7 ? 4u : 3u) &&
                      st.k[1] == st.r - st.k[0] && (lgV == 0 || lgV == 2);
    return full ? st.r : 0u;
}

// f(b0, nb) over a batch in chunks of at most MAX_BATCH columns, until one returns an error
template <class F> inline int split_batch(uint32_t batch, F f) {
    for (uint32_t b0 = 0; b0 < batch; b0 += MAX_BATCH) {
        const int rc = f(b0, batch - b0 < MAX_BATCH ? batch - b0 : MAX_BATCH);
        if (rc) return rc;
    }
    return 0;
}

}  // namespace lw
