// Library context: device selection, error plumbing, twiddle caches, scratch memory.
// The reference creates and drops all device state per call (math/src/fft/gpu/cuda/polynomial.rs:21,37);
// here it is built once and reused.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <mutex>
#include <shared_mutex>
#include <string>
#include <vector>
#include "../../include/lw_hip.h"

namespace lw {

void set_error(const char *fmt, ...);
// Diagnostic / A-B switches (LW_HIP_MSM_C, LW_HIP_SRS_FOLD, ...) are honoured only in processes started with
// LW_HIP_TUNING=1 (read once): a stray variable in a prover's environment cannot change the schedule.
const char *tuning_env(const char *name);
extern thread_local std::string g_last_error;

#define LW_HIP_CHECK(expr, code)                                                            \
    do {                                                                                    \
        hipError_t _e = (expr);                                                             \
        if (_e != hipSuccess) {                                                             \
            ::lw::set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, __LINE__); \
            return (code);                                                                  \
        }                                                                                   \
    } while (0)

struct DeviceBuf {
    void *p = nullptr;
    size_t bytes = 0;
    int ensure(size_t need);   // grow-only; returns LW_OK / LW_ERR_ALLOC
    void release();
};

struct TwiddleTable {
    DeviceBuf buf;
    uint32_t log_n = 0;   // table holds 2^(log_n-1) entries; prefix property serves every smaller size
    bool valid = false;
};

struct CosetCache {
    DeviceBuf lo, hi;
    uint32_t hbits = 0;
    uint32_t hi_bits = 0;
    uint32_t words[8] = {0};
    int field = -1;
    bool inverse = false;
    bool fold_ninv = false;
    bool valid = false;
};

struct ProfSpan {
    const char *name;
    hipEvent_t e0, e1;
};

// State shared by all lanes (below): the twiddle tables (256 MiB per field and direction at 2^24 — not something to keep
// per lane) and the lock that separates ordinary calls from the operations that touch every lane.
//   rw held SHARED  by every entry point for the duration of its call (it may hold table pointers, lane buffers);
//   rw held UNIQUE  by init / shutdown / profile begin + end / timings, and while a twiddle table is rebuilt: then no call is
//                   running, so the old table can be freed (hipFree also drains the device) and every lane may be touched.
struct SharedState {
    std::shared_mutex rw;
    TwiddleTable tw[3][2];   // [field][dir]
    // Circle FFT over Mersenne31 (circle.hip), same discipline (ensure_twiddle_table below).  Each buffer holds the
    // evaluation twiddles in its first half and their inverses (interpolation) in the second.
    TwiddleTable circle_x;       // the x-layers 0 .. log_n - 2, layer i at word 2^i - 1: they do not depend on the size
    TwiddleTable circle_y[31];   // [log2n]: the last (y) layer of that size, 2^(log2n - 1) words
    // Goldilocks NTT (goldilocks.hip), same discipline: [dir], T[g] = w^bitrev(g) for the primitive 2^32-th root
    // goldilocks_root (0: none yet).  One root at a time: a call with another root invalidates both tables.
    TwiddleTable goldilocks[2];
    uint64_t goldilocks_root = 0;
    // Pedersen lookup tables (pedersen.hip): a __device__ array of the library, filled once per device under rw held unique
    bool pedersen_table_ready = false;
    // Monolith constants (monolith.hip): a __constant__ table of the library for every (width, rounds), same discipline
    bool monolith_table_ready = false;
    bool initialised = false;
    int device = -1;
};
SharedState &shared_state();

// One LANE of the library: everything a call scribbles on (scratch, staging, MSM workspace, side streams, the cross-stream
// ordering event).  A call takes the first lane whose lock is free, so calls from different host threads — the reference's
// rayon loop over columns, provers/stark/src/trace.rs:186-190, or an NTT caller beside an MSM caller — run CONCURRENTLY on
// different lanes (one caller's download overlaps the other's upload and kernels); a single-threaded caller always gets
// lane 0 and sees exactly the behaviour of a one-context library.  Lanes allocate lazily: memory grows with the
// concurrency actually used.
constexpr int LW_LANES = 4;

struct Context {
    bool profiling = false;
    std::vector<ProfSpan> spans;
    std::vector<hipEvent_t> event_pool;
    // record a begin/end event pair around one kernel launch when profiling
    hipEvent_t prof_begin(hipStream_t s);
    void prof_end(const char *name, hipEvent_t e0, hipStream_t s);

    bool initialised = false;   // mirrors of SharedState (set for every lane by init)
    int device = -1;
    std::mutex mu;
    TwiddleTable (&tw)[3][2] = shared_state().tw;   // shared by all lanes; rebuilt only under SharedState::rw held unique
    std::shared_lock<std::shared_mutex> *call_lock = nullptr;   // the running call's shared hold on SharedState::rw (Entry)
    DeviceBuf bb_coset;      // two-level power tables of the current BabyBear coset offset (rebuilt per call: 8192 exponentiations)
    DeviceBuf gl_coset;      // the same for the current Goldilocks coset offset (goldilocks.hip), u64 entries
    DeviceBuf scratch;
    DeviceBuf small;         // staging for small power tables
    CosetCache coset[3];     // forward coset, inverse coset, multi-GPU cross-step twiddle base
    DeviceBuf msm_ws;
    uint32_t *pinned_words = nullptr;   // 64 pinned host words: small device -> host results read while other streams run (msm_core.cuh)
    DeviceBuf msm_scalars;   // canonical scalars when the caller hands Montgomery-form FrElements
    DeviceBuf msm_prefix;    // running products of the batch inversion (msm_to_affine_kernel), one base-field element per point
    DeviceBuf msm_affine;    // per-call affine copy of a large projective point set (msm_device)
    hipStream_t aux_stream = nullptr;   // side stream: the normalisation of the points runs beside the scalar sort
    hipStream_t aux_hi = nullptr;       // high-priority side stream: short kernels that must get CU slots UNDER a long-running kernel of the caller's stream
    hipEvent_t aux_fork = nullptr, aux_join = nullptr;
    DeviceBuf host_io_a, host_io_b;   // device staging for the host-buffer entry points
    hipStream_t io_stream = nullptr;  // ... and the stream they run on
    DeviceBuf pipe_tmp;               // intermediates of the device-resident pipelines (FRI layer evaluation, Groth16 cosets)
    DeviceBuf poly_ws;                // polynomial evaluation / division: tile sums, carries, totals (poly.hip)
    DeviceBuf poly_q;                 // the quotient a KZG opening commits (canonical scalars for the SRS MSM)
    // DEEP composition (poly.hip): pinned host staging of the call's tables, and the event after which the device has
    // read it (a call that hands no host result back returns while its upload is still in flight)
    void *deep_pin = nullptr;
    size_t deep_pin_bytes = 0;
    hipEvent_t deep_pin_read = nullptr;
    lw_timings_t timings = {};
    // Cross-stream ordering of the context-owned buffers (scratch, tables, staging, MSM workspace): every entry point
    // records `order_event` on its launch stream when it returns; a call arriving on a different stream first makes
    // that stream wait for it.  (c.mu only serialises the host side.)
    hipEvent_t order_event = nullptr;
    hipStream_t last_stream = nullptr;
    bool have_last = false;
    DeviceBuf shard_a, shard_b;       // exchange buffers of the sharded (multi-GPU) entry points
    DeviceBuf shard_c;                // (S, A) pairs of the sharded MSM's all-gather
    uint64_t shard_prepared_key = 0;  // shape of the last sharded NTT whose allocations every rank agreed on (comm.hip)
    std::vector<hipEvent_t> sync_pool;   // untimed events for cross-stream dependencies inside one call
    void release_all();               // frees every cached device object (shutdown / device change)
};

// Held by every extern "C" entry point for its whole duration: context lock, lazy init, device binding (the HIP
// current device is per thread) and the cross-stream ordering above.
struct Entry {
    // Lock order: the lane first, SharedState::rw second.  (A caller waiting for a lane must not hold rw: the lane's owner may be
    // waiting to upgrade its own hold to exclusive, which needs every shared holder out.)
    std::unique_lock<std::mutex> lock;            // the lane's lock
    Context &c;
    std::shared_lock<std::shared_mutex> shared;   // SharedState::rw, shared
    hipStream_t stream;
    int rc = LW_OK;
    int prev_device = -1;
    // lane0: the call uses process-wide state that lives with lane 0 (the RCCL communicator and its exchange buffers)
    explicit Entry(void *hip_stream, bool lane0 = false);
    // Host-buffer entry points: switch the call to the lane's own (non-blocking) stream instead of the null stream, so that
    // calls running on different lanes do not serialise on it; returns the stream (nullptr + rc set on failure).
    hipStream_t use_lane_stream();
    ~Entry();
    Entry(const Entry &) = delete;
};
// Upgrade of the running call's hold on SharedState::rw to exclusive for the duration of a scope (twiddle rebuild): releases
// the shared hold first — other calls drain — and takes it back afterwards.  Re-check the condition after construction.
struct ExclusiveScope {
    Context &c;
    explicit ExclusiveScope(Context &cc) : c(cc) {
        if (c.call_lock) c.call_lock->unlock();
        shared_state().rw.lock();
    }
    ~ExclusiveScope() {
        shared_state().rw.unlock();
        if (c.call_lock) c.call_lock->lock();
    }
};

// The cache skeleton of the shared twiddle tables (ntt256.hip, ntt_bb.hip): `t` serves every transform of up to 2^t.log_n
// points once valid.  Otherwise it is rebuilt for 2^L points, L = max(log2n, 16) — so that small transforms never trigger a
// rebuild storm — unless the field has no root of that order.  The tables are shared by all lanes: (re)building one needs
// every other call out of the library (the old table is freed), so the call's shared hold is given up for the scope and
// taken back afterwards; another lane may have built the table in between.  fill(L) enqueues on `stream` whatever writes
// the 2^(L-1) entries of entry_bytes each into t.buf and returns LW_OK or an error code.  The table is marked invalid
// before its buffer is touched and valid only once the fill has completed: a failed rebuild leaves no lane a stale table.
template <class Fill>
int ensure_twiddle_table(Context &c, TwiddleTable &t, uint32_t log2n, uint32_t two_adicity, size_t entry_bytes, hipStream_t stream,
                         Fill fill) {
    if (t.valid && t.log_n >= log2n) return LW_OK;
    if (log2n < 1) return LW_OK;
    ExclusiveScope excl(c);
    if (t.valid && t.log_n >= log2n) return LW_OK;
    uint32_t L = log2n < 16 ? 16 : log2n;
    if (L > two_adicity) L = log2n;
    t.valid = false;
    if (t.buf.ensure(((size_t)1 << (L - 1)) * entry_bytes)) return LW_ERR_ALLOC;
    const int rc = fill(L);
    if (rc) return rc;
    LW_HIP_CHECK(hipGetLastError(), LW_ERR_LAUNCH);
    LW_HIP_CHECK(hipStreamSynchronize(stream), LW_ERR_LAUNCH);
    t.log_n = L;
    t.valid = true;
    return LW_OK;
}

Context &lane(int i);
inline Context &ctx() { return lane(0); }
int ensure_init();

}  // namespace lw
