// Polynomial evaluation and Ruffini division on the device (Polynomial::evaluate, math/src/polynomial/mod.rs:98-109;
// ruffini_division_inplace, :157-164) and the KZG openings built on them (KateZaveruchaGoldberg::open / open_batch,
// crypto/src/commitments/kzg.rs:171-180, 206-226).
//
// Division by (X - x) is the first-order linear recurrence  c_n = 0,  c_i = a_i + x c_{i+1}:  the quotient is
// q_{i-1} = c_i (i = 1 .. n-1) and the remainder c_0 = p(x).  It runs as a reduce-then-scan in three launches, whatever n:
//   1. poly_tile_reduce_kernel  every tile of TILE = 256 threads x E coefficients computes its Horner sum with carry-in 0,
//                               S_t = sum_{i in tile} a_i x^(i - tT)  (each thread folds E consecutive coefficients, the block
//                               combines the 256 partial sums with an LDS suffix scan under x^E, x^2E, ...).  Evaluation
//                               of K polynomials at M points is this kernel plus step 2 and nothing else.
//   2. poly_tile_scan_kernel    one block per series: c at the top of every tile, C_t = S_t + x^T C_{t+1}, as a suffix scan
//                               over the tile sums (each thread a contiguous group of tiles, then an LDS scan under x^(TG));
//                               the series' total is p(x).
//   3. poly_tile_rescan_kernel  every tile rescans with its carry and stores q.
// open_batch's fold sum_k u^k p_k is formed where the coefficients are loaded (step 3) and on the tile sums (step 2, by
// linearity), so the combined polynomial never exists in memory.  Every stored value is fully reduced: fe_add / fe_mul
// return canonical residues for canonical operands, including Stark252 (LAZY applies to the NTT butterflies only).
#include <string.h>
#include <vector>
#include "internal.h"
#include "field.cuh"

namespace lw {

constexpr int POLY_THREADS = 256;
constexpr int POLY_E = 8;                                             // consecutive coefficients per thread
constexpr uint64_t POLY_TILE = (uint64_t)POLY_THREADS * POLY_E;      // 2048 coefficients per block
constexpr int POLY_PTS = 4;                                           // evaluation points per launch
constexpr int POLY_NPOW = 10;                                         // z, z^E, z^2E, ..., z^256E = z^TILE

struct PolyRef {
    const void *p;
    uint64_t len;
};

// Everything a launch needs travels as its kernel argument: the power tables of up to POLY_PTS points are computed on
// the host, so that a device-form call with no host result has nothing in flight that reads caller memory.
template <class F>
struct PolyArgs {
    PolyRef one;              // the polynomial when tab == nullptr (k == 1)
    const PolyRef *tab;       // k polynomials (device copy of the caller's table)
    uint32_t k, m;            // polynomials; points of this launch
    uint32_t blk0;            // scan: first series of this launch (k * m = the folded division series)
    uint32_t vals_stride, vals_j0;   // scan: total of series (kk, j) goes to vals[kk * vals_stride + vals_j0 + j]
    uint64_t ntiles;
    uint64_t n;               // division: length of the folded polynomial
    char *sums;               // [k][m][ntiles] tile sums
    char *carries;            // [ntiles] c at the top of every tile (division)
    char *vals;               // series totals
    char *q;                  // quotient, n - 1 elements
    Fe<F> ups;                // open_batch fold factor
    Fe<F> pw[POLY_PTS][POLY_NPOW];
};

template <class F>
__device__ __forceinline__ PolyRef poly_ref(const PolyArgs<F> &a, uint32_t k) { return a.tab ? a.tab[k] : a.one; }

template <class F>
__device__ __forceinline__ Fe<F> poly_coeff(const PolyRef &r, uint64_t i) {
    return i < r.len ? fe_load<F>((const char *)r.p + i * 32) : Fe<F>::zero();
}

// sum_k u^k p_k[i] (Horner over k)
template <class F>
__device__ __forceinline__ Fe<F> poly_folded(const PolyArgs<F> &a, uint64_t i) {
    Fe<F> v = poly_coeff<F>(poly_ref(a, a.k - 1), i);
    for (int k = (int)a.k - 2; k >= 0; k--) v = fe_add<F>(fe_mul<F>(v, a.ups), poly_coeff<F>(poly_ref(a, (uint32_t)k), i));
    return v;
}

// inclusive suffix scan over the block's 256 threads: v_r <- sum_{r' >= r} w^(r' - r) v_r', pw(s) = w^(2^s).
// On return lds[r] holds every thread's inclusive value.
template <class F, class Pow>
__device__ __forceinline__ Fe<F> block_suffix_scan(Fe<F> v, Fe<F> *lds, const Pow &pw) {
    const int r = threadIdx.x;
#pragma unroll 1
    for (int s = 0; s < 8; s++) {
        lds[r] = v;
        __syncthreads();
        const int d = 1 << s;
        if (r + d < POLY_THREADS) v = fe_add<F>(v, fe_mul<F>(pw(s), lds[r + d]));
        __syncthreads();
    }
    lds[r] = v;
    __syncthreads();
    return v;
}

// 1. tile sums of polynomial blockIdx.y at every point of the launch
template <class F>
__global__ __launch_bounds__(POLY_THREADS) void poly_tile_reduce_kernel(const PolyArgs<F> a) {
    __shared__ Fe<F> lds[POLY_THREADS];
    const uint32_t k = blockIdx.y;
    const uint64_t t = blockIdx.x;
    const PolyRef pr = poly_ref(a, k);
    char *out = a.sums + ((uint64_t)k * a.m * a.ntiles + t) * 32;
    if (t * POLY_TILE >= pr.len) {   // past the end of this polynomial: its tiles sum to zero
        if (threadIdx.x < a.m) fe_store<F>(out + (uint64_t)threadIdx.x * a.ntiles * 32, Fe<F>::zero());
        return;
    }
    const uint64_t base = t * POLY_TILE + (uint64_t)threadIdx.x * POLY_E;
    Fe<F> c[POLY_E];
#pragma unroll
    for (int e = 0; e < POLY_E; e++) c[e] = poly_coeff<F>(pr, base + e);
#pragma unroll 1
    for (uint32_t j = 0; j < a.m; j++) {
        const Fe<F> z = a.pw[j][0];
        Fe<F> h = c[POLY_E - 1];
#pragma unroll
        for (int e = POLY_E - 2; e >= 0; e--) h = fe_add<F>(fe_mul<F>(h, z), c[e]);
        h = block_suffix_scan<F>(h, lds, [&](int s) { return a.pw[j][1 + s]; });
        if (threadIdx.x == 0) fe_store<F>(out + (uint64_t)j * a.ntiles * 32, h);
    }
}

// 2. one block per series: series b < k * m is polynomial b / m at point b % m (its total is the evaluation); series
// k * m is the u-fold of every polynomial's tile sums at point 0, whose carries feed the rescan (division).
template <class F>
__global__ __launch_bounds__(POLY_THREADS) void poly_tile_scan_kernel(const PolyArgs<F> a) {
    __shared__ Fe<F> lds[POLY_THREADS];
    __shared__ Fe<F> mul[8];
    const uint32_t b = blockIdx.x + a.blk0;
    const bool fold = b == a.k * a.m;
    const uint32_t j = fold ? 0 : b % a.m;
    const Fe<F> P = a.pw[j][POLY_NPOW - 1];   // x^TILE
    const uint64_t nt = a.ntiles, G = (nt + POLY_THREADS - 1) / POLY_THREADS, t0 = (uint64_t)threadIdx.x * G;
    auto tile = [&](uint64_t t) -> Fe<F> {
        if (t >= nt) return Fe<F>::zero();
        if (!fold) return fe_load<F>(a.sums + ((uint64_t)b * nt + t) * 32);
        Fe<F> v = fe_load<F>(a.sums + ((uint64_t)(a.k - 1) * a.m * nt + t) * 32);
        for (int k = (int)a.k - 2; k >= 0; k--) v = fe_add<F>(fe_mul<F>(v, a.ups), fe_load<F>(a.sums + ((uint64_t)k * a.m * nt + t) * 32));
        return v;
    };
    if (threadIdx.x == 0) {   // neighbouring groups are x^(TILE G) apart
        Fe<F> w = fe_pow_u64<F>(P, G);
        for (int s = 0; s < 8; s++) {
            mul[s] = w;
            w = fe_sqr<F>(w);
        }
    }
    Fe<F> acc = Fe<F>::zero();
#pragma unroll 1
    for (uint64_t g = G; g-- > 0;) acc = fe_add<F>(fe_mul<F>(acc, P), tile(t0 + g));
    __syncthreads();
    acc = block_suffix_scan<F>(acc, lds, [&](int s) { return mul[s]; });
    if (threadIdx.x == 0) {
        const uint32_t kk = fold ? a.k : b / a.m;
        fe_store<F>(a.vals + ((uint64_t)kk * a.vals_stride + a.vals_j0 + j) * 32, acc);
    }
    if (!fold) return;
    Fe<F> c = threadIdx.x + 1 < POLY_THREADS ? lds[threadIdx.x + 1] : Fe<F>::zero();   // c at the top of this group
#pragma unroll 1
    for (uint64_t g = G; g-- > 0;) {
        const uint64_t t = t0 + g;
        if (t < nt) fe_store<F>(a.carries + t * 32, c);
        c = fe_add<F>(fe_mul<F>(c, P), tile(t));
    }
}

// 3. rescan of every tile with its carry; CANON stores representative() (the scalars of a KZG commitment)
template <class F, bool CANON>
__global__ __launch_bounds__(POLY_THREADS) void poly_tile_rescan_kernel(const PolyArgs<F> a) {
    __shared__ Fe<F> lds[POLY_THREADS];
    const uint64_t t = blockIdx.x;
    const uint64_t base = t * POLY_TILE + (uint64_t)threadIdx.x * POLY_E;
    const Fe<F> x = a.pw[0][0];
    Fe<F> c[POLY_E];
#pragma unroll
    for (int e = 0; e < POLY_E; e++) c[e] = base + e < a.n ? poly_folded<F>(a, base + e) : Fe<F>::zero();
    Fe<F> h = c[POLY_E - 1];
#pragma unroll
    for (int e = POLY_E - 2; e >= 0; e--) h = fe_add<F>(fe_mul<F>(h, x), c[e]);
    const Fe<F> top = fe_load<F>(a.carries + t * 32);
    if (threadIdx.x == POLY_THREADS - 1) h = fe_add<F>(h, fe_mul<F>(a.pw[0][1], top));
    block_suffix_scan<F>(h, lds, [&](int s) { return a.pw[0][1 + s]; });
    Fe<F> v = threadIdx.x + 1 < POLY_THREADS ? lds[threadIdx.x + 1] : top;   // c just above this thread's coefficients
#pragma unroll
    for (int e = POLY_E - 1; e >= 0; e--) {
        v = fe_add<F>(c[e], fe_mul<F>(x, v));
        const uint64_t i = base + e;
        if (i >= 1 && i < a.n) fe_store<F>(a.q + (i - 1) * 32, CANON ? fe_from_mont<F>(v) : v);
    }
}

// ---- DEEP composition: out = sum_j quot(sum_k w[k][j] p_k, x_j) (lw_stark_deep_composition) ----
// The same three steps over a K x M weight matrix, POLY_PTS points (a "group") per round of launches:
//   1. deep_tile_reduce_kernel  tile sums of every (polynomial, point) pair with a non-zero weight; the coefficients are
//                               loaded once for the points of the group.  Only the tile's total is needed, so the 256
//                               partial sums are folded as a tree (128 + 64 + ... + 1 products), not scanned.
//   2. deep_tile_scan_kernel    one block per series: per point the w-weighted fold of the pairs' tile sums (carries),
//                               and per pair its own series when the values p_k(x_j) are asked for.
//   3. deep_tile_rescan_kernel  per tile, point after point: sum_k w[k][j] p_k[i] formed on load, rescanned with that
//                               point's carry, the quotient coefficients of all points added up in registers and stored
//                               once (groups after the first add to what the output holds).
// Pairs with weight zero are masked on the host: their coefficients are never read, their sums never written or read.
template <class F>
struct DeepArgs {
    const PolyRef *tab;       // k polynomials
    const uint32_t *mask;     // [k] bit j: the weight of polynomial k at point j of this group is non-zero
    const char *w;            // [POLY_PTS][k] weights of this group, point-major
    uint32_t k, mp;           // polynomials; points of this group
    uint32_t k0;              // reduce: first polynomial of this launch (blockIdx.y counts from it)
    uint32_t evals;           // scan: the per-pair series too
    uint32_t m;               // row length of vals
    uint32_t col[POLY_PTS];   // column of each group point in the caller's matrix
    uint32_t accumulate;      // rescan: add to the output
    uint64_t ntiles;
    uint64_t n;               // the longest length
    char *sums;               // [k][POLY_PTS][ntiles]
    char *carries;            // [POLY_PTS][ntiles]
    char *vals;               // [k][m] p_k(x_j)
    char *out;                // n - 1 elements
    Fe<F> pw[POLY_PTS][POLY_NPOW];
};

template <class F>
__global__ __launch_bounds__(POLY_THREADS) void deep_tile_reduce_kernel(const DeepArgs<F> a) {
    __shared__ Fe<F> lds[POLY_THREADS];
    const uint32_t k = a.k0 + blockIdx.y;
    const uint64_t t = blockIdx.x;
    const uint32_t mask = a.mask[k];
    if (!mask) return;
    const PolyRef pr = a.tab[k];
    const int r = threadIdx.x;
    char *out = a.sums + ((uint64_t)k * POLY_PTS * a.ntiles + t) * 32;
    if (t * POLY_TILE >= pr.len) {   // past the end of this polynomial: its tiles sum to zero
        if (r < (int)a.mp && (mask >> r & 1)) fe_store<F>(out + (uint64_t)r * a.ntiles * 32, Fe<F>::zero());
        return;
    }
    const uint64_t base = t * POLY_TILE + (uint64_t)r * POLY_E;
    Fe<F> c[POLY_E];
#pragma unroll
    for (int e = 0; e < POLY_E; e++) c[e] = poly_coeff<F>(pr, base + e);
#pragma unroll 1
    for (uint32_t j = 0; j < a.mp; j++) {
        if (!(mask >> j & 1)) continue;
        const Fe<F> z = a.pw[j][0];
        Fe<F> h = c[POLY_E - 1];
#pragma unroll
        for (int e = POLY_E - 2; e >= 0; e--) h = fe_add<F>(fe_mul<F>(h, z), c[e]);
        // sum_r z^(E r) h_r: the upper half of the live threads folds onto the lower half, z^(E d) apart.  A step writes
        // lds[d, 2d) and reads it back; the next one writes [d/2, d): one barrier per step is enough.
#pragma unroll 1
        for (int s = 7; s >= 0; s--) {
            const int d = 1 << s;
            if (r >= d && r < 2 * d) lds[r] = h;
            __syncthreads();
            if (r < d) h = fe_add<F>(h, fe_mul<F>(a.pw[j][1 + s], lds[r + d]));
        }
        if (r == 0) fe_store<F>(out + (uint64_t)j * a.ntiles * 32, h);
    }
}

// block b: point b % mp; b / mp == 0 is the point's weighted fold (carries), b / mp == kk + 1 the pair (kk, point)
template <class F>
__global__ __launch_bounds__(POLY_THREADS) void deep_tile_scan_kernel(const DeepArgs<F> a) {
    __shared__ Fe<F> lds[POLY_THREADS];
    __shared__ Fe<F> mul[8];
    const uint32_t j = blockIdx.x % a.mp, kb = blockIdx.x / a.mp;
    const bool fold = kb == 0;
    if (!fold && !(a.mask[kb - 1] >> j & 1)) return;
    const Fe<F> P = a.pw[j][POLY_NPOW - 1];   // x^TILE
    const uint64_t nt = a.ntiles, G = (nt + POLY_THREADS - 1) / POLY_THREADS, t0 = (uint64_t)threadIdx.x * G;
    auto tile = [&](uint64_t t) -> Fe<F> {
        if (t >= nt) return Fe<F>::zero();
        if (!fold) return fe_load<F>(a.sums + (((uint64_t)(kb - 1) * POLY_PTS + j) * nt + t) * 32);
        Fe<F> v = Fe<F>::zero();
        for (uint32_t k = 0; k < a.k; k++)
            if (a.mask[k] >> j & 1)
                v = fe_add<F>(v, fe_mul<F>(fe_load<F>(a.w + ((uint64_t)j * a.k + k) * 32),
                                           fe_load<F>(a.sums + (((uint64_t)k * POLY_PTS + j) * nt + t) * 32)));
        return v;
    };
    if (threadIdx.x == 0) {   // neighbouring groups are x^(TILE G) apart
        Fe<F> w = fe_pow_u64<F>(P, G);
        for (int s = 0; s < 8; s++) {
            mul[s] = w;
            w = fe_sqr<F>(w);
        }
    }
    Fe<F> acc = Fe<F>::zero();
#pragma unroll 1
    for (uint64_t g = G; g-- > 0;) acc = fe_add<F>(fe_mul<F>(acc, P), tile(t0 + g));
    __syncthreads();
    acc = block_suffix_scan<F>(acc, lds, [&](int s) { return mul[s]; });
    if (!fold) {
        if (threadIdx.x == 0) fe_store<F>(a.vals + ((uint64_t)(kb - 1) * a.m + a.col[j]) * 32, acc);
        return;
    }
    Fe<F> c = threadIdx.x + 1 < POLY_THREADS ? lds[threadIdx.x + 1] : Fe<F>::zero();   // c at the top of this group
#pragma unroll 1
    for (uint64_t g = G; g-- > 0;) {
        const uint64_t t = t0 + g;
        if (t < nt) fe_store<F>(a.carries + ((uint64_t)j * nt + t) * 32, c);
        c = fe_add<F>(fe_mul<F>(c, P), tile(t));
    }
}

// The running sum of the quotients of the group's points lives in LDS between points (each thread its own E slots): next to
// c[] it would take the kernel past 256 registers.  The last point adds its share and stores.
template <class F>
__global__ __launch_bounds__(POLY_THREADS) void deep_tile_rescan_kernel(const DeepArgs<F> a) {
    __shared__ Fe<F> lds[POLY_THREADS];
    __shared__ Fe<F> qs[POLY_E * POLY_THREADS];
    const uint64_t t = blockIdx.x;
    const uint64_t base = t * POLY_TILE + (uint64_t)threadIdx.x * POLY_E;
#pragma unroll 1
    for (uint32_t j = 0; j < a.mp; j++) {
        Fe<F> c[POLY_E];
#pragma unroll
        for (int e = 0; e < POLY_E; e++) c[e] = Fe<F>::zero();
#pragma unroll 1
        for (uint32_t k = 0; k < a.k; k++) {
            if (!(a.mask[k] >> j & 1)) continue;
            const PolyRef pr = a.tab[k];
            if (t * POLY_TILE >= pr.len) continue;
            const Fe<F> w = fe_load<F>(a.w + ((uint64_t)j * a.k + k) * 32);
#pragma unroll
            for (int e = 0; e < POLY_E; e++) c[e] = fe_add<F>(c[e], fe_mul<F>(w, poly_coeff<F>(pr, base + e)));
        }
        const Fe<F> x = a.pw[j][0];
        Fe<F> h = c[POLY_E - 1];
#pragma unroll
        for (int e = POLY_E - 2; e >= 0; e--) h = fe_add<F>(fe_mul<F>(h, x), c[e]);
        const Fe<F> top = fe_load<F>(a.carries + ((uint64_t)j * a.ntiles + t) * 32);
        if (threadIdx.x == POLY_THREADS - 1) h = fe_add<F>(h, fe_mul<F>(a.pw[j][1], top));
        block_suffix_scan<F>(h, lds, [&](int s) { return a.pw[j][1 + s]; });
        Fe<F> v = threadIdx.x + 1 < POLY_THREADS ? lds[threadIdx.x + 1] : top;   // c just above this thread's coefficients
        __syncthreads();   // the next point's scan writes lds
        const bool last = j + 1 == a.mp;
#pragma unroll
        for (int e = POLY_E - 1; e >= 0; e--) {
            v = fe_add<F>(c[e], fe_mul<F>(x, v));
            Fe<F> q = j ? fe_add<F>(v, qs[e * POLY_THREADS + threadIdx.x]) : v;
            if (!last) {
                qs[e * POLY_THREADS + threadIdx.x] = q;
                continue;
            }
            const uint64_t i = base + e;
            if (i >= 1 && i < a.n) {
                char *o = a.out + (i - 1) * 32;
                fe_store<F>(o, a.accumulate ? fe_add<F>(q, fe_load<F>(o)) : q);
            }
        }
    }
}

// ---- host side ----
template <class F>
static void point_powers(const void *z_ref, Fe<F> (&pw)[POLY_NPOW]) {
    alignas(16) uint64_t w[4];
    memcpy(w, z_ref, 32);
    pw[0] = fe_load<F>(w);
    pw[1] = fe_pow_u64<F>(pw[0], POLY_E);
    for (int s = 2; s < POLY_NPOW; s++) pw[s] = fe_sqr<F>(pw[s - 1]);
}
template <class F>
static Fe<F> load_ref(const void *ref) {
    alignas(16) uint64_t w[4];
    memcpy(w, ref, 32);
    return fe_load<F>(w);
}

static size_t round256(size_t b) { return (b + 255) & ~(size_t)255; }

struct PolyWs {
    char *tab, *sums, *carries, *vals;
};
// library workspace of one call: [polynomial table | tile sums | carries | totals]
static int poly_ws(Context &c, uint32_t k, uint64_t sums, uint64_t ntiles, uint64_t vals, PolyWs &w) {
    const size_t a = round256((size_t)k * sizeof(PolyRef)), b = round256(sums * 32), d = round256(ntiles * 32), e = round256(vals * 32);
    if (c.poly_ws.ensure(a + b + d + e)) return LW_ERR_ALLOC;
    w.tab = (char *)c.poly_ws.p;
    w.sums = w.tab + a;
    w.carries = w.sums + b;
    w.vals = w.carries + d;
    return LW_OK;
}
// the table goes to the device only for k > 1; those calls synchronise before they return (the host copy is read
// until then)
template <class F>
static int poly_refs(const PolyRef *refs, uint32_t k, const PolyWs &w, PolyArgs<F> &a, hipStream_t s) {
    a.k = k;
    a.one = refs[0];
    a.tab = nullptr;
    if (k > 1) {
        LW_HIP_CHECK(hipMemcpyAsync(w.tab, refs, (size_t)k * sizeof(PolyRef), hipMemcpyHostToDevice, s), LW_ERR_LAUNCH);
        a.tab = (const PolyRef *)w.tab;
    }
    return LW_OK;
}

static uint64_t tiles_of(uint64_t n) { return n ? (n + POLY_TILE - 1) / POLY_TILE : 1; }

// K x M evaluation table -> out_host[kk * m + j] (Montgomery form); synchronises
template <class F>
static int evaluate_locked(Context &c, const PolyRef *refs, uint32_t k, const void *points, uint32_t m, void *out_host, hipStream_t s) {
    uint64_t maxlen = 0;
    for (uint32_t i = 0; i < k; i++) maxlen = refs[i].len > maxlen ? refs[i].len : maxlen;
    const uint64_t nt = tiles_of(maxlen);
    PolyWs w;
    if (poly_ws(c, k, (uint64_t)k * POLY_PTS * nt, 0, (uint64_t)k * m, w)) return LW_ERR_ALLOC;
    PolyArgs<F> a;
    memset(&a, 0, sizeof(a));
    int rc = poly_refs<F>(refs, k, w, a, s);
    if (rc) return rc;
    a.ntiles = nt;
    a.sums = w.sums;
    a.vals = w.vals;
    a.vals_stride = m;
    for (uint32_t j0 = 0; j0 < m; j0 += POLY_PTS) {
        a.m = m - j0 < (uint32_t)POLY_PTS ? m - j0 : (uint32_t)POLY_PTS;
        a.vals_j0 = j0;
        for (uint32_t j = 0; j < a.m; j++) point_powers<F>((const char *)points + (size_t)(j0 + j) * 32, a.pw[j]);
        hipEvent_t pe = c.prof_begin(s);
        hipLaunchKernelGGL((poly_tile_reduce_kernel<F>), dim3((uint32_t)nt, k), dim3(POLY_THREADS), 0, s, a);
        c.prof_end("poly_tile_reduce_kernel", pe, s);
        pe = c.prof_begin(s);
        hipLaunchKernelGGL((poly_tile_scan_kernel<F>), dim3(k * a.m), dim3(POLY_THREADS), 0, s, a);
        c.prof_end("poly_tile_scan_kernel", pe, s);
        LW_HIP_CHECK(hipGetLastError(), LW_ERR_LAUNCH);
    }
    LW_HIP_CHECK(hipMemcpyAsync(out_host, w.vals, (size_t)k * m * 32, hipMemcpyDeviceToHost, s), LW_ERR_LAUNCH);
    LW_HIP_CHECK(hipStreamSynchronize(s), LW_ERR_LAUNCH);
    return LW_OK;
}

// quotient of sum_kk u^kk p_kk by (X - x) -> d_q (n - 1 elements, n = the longest length); evals_host: the k values
// p_kk(x); rem_host: the folded remainder.  Synchronises when a host result is asked for.
template <class F, bool CANON>
static int divide_locked(Context &c, const PolyRef *refs, uint32_t k, const void *x, const void *ups, void *d_q, void *evals_host,
                         void *rem_host, hipStream_t s) {
    uint64_t n = 0;
    for (uint32_t i = 0; i < k; i++) n = refs[i].len > n ? refs[i].len : n;
    if (n == 0) {   // the zero polynomial: empty quotient, p(x) = 0
        if (evals_host) memset(evals_host, 0, (size_t)k * 32);
        if (rem_host) memset(rem_host, 0, 32);
        return LW_OK;
    }
    const uint64_t nt = tiles_of(n);
    PolyWs w;
    if (poly_ws(c, k, (uint64_t)k * nt, nt, (uint64_t)k + 1, w)) return LW_ERR_ALLOC;
    PolyArgs<F> a;
    memset(&a, 0, sizeof(a));
    int rc = poly_refs<F>(refs, k, w, a, s);
    if (rc) return rc;
    a.m = 1;
    a.ntiles = nt;
    a.n = n;
    a.sums = w.sums;
    a.carries = w.carries;
    a.vals = w.vals;
    a.vals_stride = 1;
    a.q = (char *)d_q;
    a.ups = k > 1 ? load_ref<F>(ups) : Fe<F>::zero();
    point_powers<F>(x, a.pw[0]);
    a.blk0 = evals_host ? 0 : k;   // the per-polynomial series only when their values are asked for
    hipEvent_t pe = c.prof_begin(s);
    hipLaunchKernelGGL((poly_tile_reduce_kernel<F>), dim3((uint32_t)nt, k), dim3(POLY_THREADS), 0, s, a);
    c.prof_end("poly_tile_reduce_kernel", pe, s);
    pe = c.prof_begin(s);
    hipLaunchKernelGGL((poly_tile_scan_kernel<F>), dim3(k + 1 - a.blk0), dim3(POLY_THREADS), 0, s, a);
    c.prof_end("poly_tile_scan_kernel", pe, s);
    if (n > 1) {
        pe = c.prof_begin(s);
        hipLaunchKernelGGL((poly_tile_rescan_kernel<F, CANON>), dim3((uint32_t)nt), dim3(POLY_THREADS), 0, s, a);
        c.prof_end("poly_tile_rescan_kernel", pe, s);
    }
    LW_HIP_CHECK(hipGetLastError(), LW_ERR_LAUNCH);
    if (evals_host) LW_HIP_CHECK(hipMemcpyAsync(evals_host, w.vals, (size_t)k * 32, hipMemcpyDeviceToHost, s), LW_ERR_LAUNCH);
    if (rem_host) LW_HIP_CHECK(hipMemcpyAsync(rem_host, w.vals + (size_t)k * 32, 32, hipMemcpyDeviceToHost, s), LW_ERR_LAUNCH);
    if (evals_host || rem_host) LW_HIP_CHECK(hipStreamSynchronize(s), LW_ERR_LAUNCH);
    return LW_OK;
}

static bool elem_is_zero(const void *e) {
    static const char z[32] = {0};
    return memcmp(e, z, 32) == 0;
}

// pinned host memory for the tables of a DEEP call (and of lw_stark_open_trees_device, stark_query.hip); the previous
// call's upload has been read once deep_pin_read fires
int deep_pin(Context &c, size_t bytes) {
    if (c.deep_pin_read) LW_HIP_CHECK(hipEventSynchronize(c.deep_pin_read), LW_ERR_LAUNCH);
    else LW_HIP_CHECK(hipEventCreateWithFlags(&c.deep_pin_read, hipEventDisableTiming), LW_ERR_ALLOC);
    if (c.deep_pin_bytes >= bytes) return LW_OK;
    if (c.deep_pin) (void)hipHostFree(c.deep_pin);
    c.deep_pin = nullptr;
    c.deep_pin_bytes = 0;
    LW_HIP_CHECK(hipHostMalloc(&c.deep_pin, bytes, hipHostMallocDefault), LW_ERR_ALLOC);
    c.deep_pin_bytes = bytes;
    return LW_OK;
}

// sum_j quot(sum_k w[k][j] p_k, x_j) -> d_out (n - 1 elements, n = the longest length > 1); evals_host: the k x m table
// of p_k(x_j) (0 where the weight is 0); len_host: the stripped length.  Synchronises when a host result is asked for.
template <class F>
static int deep_locked(Context &c, const PolyRef *refs, uint32_t k, const void *points, uint32_t m, const void *weights, void *d_out,
                       size_t *len_host, void *evals_host, hipStream_t s) {
    uint64_t n = 0;
    for (uint32_t i = 0; i < k; i++) n = refs[i].len > n ? refs[i].len : n;
    const uint64_t nt = tiles_of(n);
    const char *W = (const char *)weights;
    std::vector<uint32_t> cols;   // the points that carry any weight
    for (uint32_t j = 0; j < m; j++)
        for (uint32_t i = 0; i < k; i++)
            if (!elem_is_zero(W + ((size_t)i * m + j) * 32)) {
                cols.push_back(j);
                break;
            }
    const size_t groups = (cols.size() + POLY_PTS - 1) / POLY_PTS;
    // tables: [polynomials | per group: masks, weights]; workspace after them: [tile sums | carries | values | length]
    const size_t tab_b = round256((size_t)k * sizeof(PolyRef)), mask_b = round256((size_t)k * 4), w_b = round256((size_t)POLY_PTS * k * 32);
    const size_t tables = tab_b + groups * (mask_b + w_b);
    const size_t sums_b = round256((size_t)k * POLY_PTS * nt * 32), car_b = round256((size_t)POLY_PTS * nt * 32);
    const size_t vals_b = round256(evals_host ? (size_t)k * m * 32 : 0);
    if (c.poly_ws.ensure(tables + sums_b + car_b + vals_b + 256)) return LW_ERR_ALLOC;
    char *d_tab = (char *)c.poly_ws.p, *d_sums = d_tab + tables, *d_car = d_sums + sums_b, *d_vals = d_car + car_b, *d_len = d_vals + vals_b;
    int rc = deep_pin(c, tables);
    if (rc) return rc;
    char *h = (char *)c.deep_pin;
    memset(h, 0, tables);
    memcpy(h, refs, (size_t)k * sizeof(PolyRef));
    for (size_t g = 0; g < groups; g++) {
        uint32_t *mask = (uint32_t *)(h + tab_b + g * (mask_b + w_b));
        char *w = (char *)mask + mask_b;
        for (uint32_t jj = 0; jj < (uint32_t)POLY_PTS && g * POLY_PTS + jj < cols.size(); jj++) {
            const uint32_t j = cols[g * POLY_PTS + jj];
            for (uint32_t i = 0; i < k; i++) {
                const char *e = W + ((size_t)i * m + j) * 32;
                if (elem_is_zero(e)) continue;
                mask[i] |= 1u << jj;
                memcpy(w + ((size_t)jj * k + i) * 32, e, 32);
            }
        }
    }
    LW_HIP_CHECK(hipMemcpyAsync(d_tab, h, tables, hipMemcpyHostToDevice, s), LW_ERR_LAUNCH);
    LW_HIP_CHECK(hipEventRecord(c.deep_pin_read, s), LW_ERR_LAUNCH);
    if (evals_host) LW_HIP_CHECK(hipMemsetAsync(d_vals, 0, (size_t)k * m * 32, s), LW_ERR_LAUNCH);
    if (!groups) LW_HIP_CHECK(hipMemsetAsync(d_out, 0, (size_t)(n - 1) * 32, s), LW_ERR_LAUNCH);   // every weight is zero
    DeepArgs<F> a;
    memset(&a, 0, sizeof(a));
    a.tab = (const PolyRef *)d_tab;
    a.k = k;
    a.m = m;
    a.evals = evals_host ? 1 : 0;
    a.ntiles = nt;
    a.n = n;
    a.sums = d_sums;
    a.carries = d_car;
    a.vals = d_vals;
    a.out = (char *)d_out;
    for (size_t g = 0; g < groups; g++) {
        a.mask = (const uint32_t *)(d_tab + tab_b + g * (mask_b + w_b));
        a.w = (const char *)a.mask + mask_b;
        a.mp = (uint32_t)(cols.size() - g * POLY_PTS < (size_t)POLY_PTS ? cols.size() - g * POLY_PTS : (size_t)POLY_PTS);
        a.accumulate = g > 0;
        for (uint32_t jj = 0; jj < a.mp; jj++) {
            a.col[jj] = cols[g * POLY_PTS + jj];
            point_powers<F>((const char *)points + (size_t)a.col[jj] * 32, a.pw[jj]);
        }
        for (uint32_t k0 = 0; k0 < k; k0 += 65535) {   // the grid's y extent
            a.k0 = k0;
            hipEvent_t pe = c.prof_begin(s);
            hipLaunchKernelGGL((deep_tile_reduce_kernel<F>), dim3((uint32_t)nt, k - k0 < 65535 ? k - k0 : 65535), dim3(POLY_THREADS), 0, s, a);
            c.prof_end("deep_tile_reduce_kernel", pe, s);
        }
        hipEvent_t pe = c.prof_begin(s);
        hipLaunchKernelGGL((deep_tile_scan_kernel<F>), dim3(a.mp * (1 + (a.evals ? k : 0))), dim3(POLY_THREADS), 0, s, a);
        c.prof_end("deep_tile_scan_kernel", pe, s);
        pe = c.prof_begin(s);
        hipLaunchKernelGGL((deep_tile_rescan_kernel<F>), dim3((uint32_t)nt), dim3(POLY_THREADS), 0, s, a);
        c.prof_end("deep_tile_rescan_kernel", pe, s);
        LW_HIP_CHECK(hipGetLastError(), LW_ERR_LAUNCH);
    }
    uint64_t len = 0;
    if (len_host) {
        rc = stripped_length_device(d_out, n - 1, (uint64_t *)d_len, s);
        if (rc) return rc;
        LW_HIP_CHECK(hipMemcpyAsync(&len, d_len, 8, hipMemcpyDeviceToHost, s), LW_ERR_LAUNCH);
    }
    if (evals_host) LW_HIP_CHECK(hipMemcpyAsync(evals_host, d_vals, (size_t)k * m * 32, hipMemcpyDeviceToHost, s), LW_ERR_LAUNCH);
    if (len_host || evals_host) LW_HIP_CHECK(hipStreamSynchronize(s), LW_ERR_LAUNCH);
    if (len_host) *len_host = (size_t)len;
    return LW_OK;
}

static bool poly_field_ok(lw_field_t f) {
    if (f == LW_FIELD_STARK252 || f == LW_FIELD_BLS12_381_FR) return true;
    set_error("field %d: polynomial evaluation and division take STARK252 or BLS12_381_FR (4 x u64 limbs)", (int)f);
    return false;
}
static bool aligned16(const void *p) { return ((uintptr_t)p & 15) == 0; }
static constexpr uint64_t POLY_MAX_LEN = (uint64_t)1 << 36;   // the grid's tile index stays below 2^31

// the scalar field of an SRS curve, or -1
static int kzg_scalar_field(lw_curve_t curve) {
    switch (curve) {
        case LW_CURVE_BLS12_381_G1: case LW_CURVE_BLS12_381_G2: return 1;   // Fr381
        case LW_CURVE_BN254_G1: case LW_CURVE_BN254_G2: return 2;           // Fr254
        default: return -1;
    }
}

// KZG open of sum_kk u^kk p_kk at x under an Entry: quotient (canonical) into library memory, then the SRS MSM
static int kzg_open_locked(Context &c, const lw_srs_t *srs, const PolyRef *refs, uint32_t k, const void *x, const void *ups,
                           void *out_proof, void *evals_host, void *eval_host, hipStream_t s) {
    uint64_t n = 0;
    for (uint32_t i = 0; i < k; i++) n = refs[i].len > n ? refs[i].len : n;
    const uint64_t nq = n ? n - 1 : 0;
    if (c.poly_q.ensure(nq ? nq * 32 : 256)) return LW_ERR_ALLOC;
    int rc = LW_OK;
    if (k) {
        rc = kzg_scalar_field(srs_curve(srs)) == 1
                 ? divide_locked<Fr381, true>(c, refs, k, x, ups, c.poly_q.p, evals_host, eval_host, s)
                 : divide_locked<Fr254, true>(c, refs, k, x, ups, c.poly_q.p, evals_host, eval_host, s);
        if (rc) return rc;
    }
    return msm_srs_locked(c, srs, (const uint64_t *)c.poly_q.p, nq, out_proof, s, 0);
}

// checks shared by the KZG entry points; returns the longest length in *n
static int kzg_check(const lw_srs_t *srs, const void *const *polys, const size_t *lens, uint32_t k, const void *x, const void *ups,
                     const void *out_proof, bool device, uint64_t *n) {
    if (!srs || !x || !out_proof || (k && (!polys || !lens)) || (k > 1 && !ups)) { set_error("null argument"); return LW_ERR_BAD_ARG; }
    if (kzg_scalar_field(srs_curve(srs)) < 0) { set_error("SRS curve %d has no KZG scalar field here", (int)srs_curve(srs)); return LW_ERR_BAD_ARG; }
    *n = 0;
    for (uint32_t i = 0; i < k; i++) {
        if (lens[i] && (!polys[i] || (device && !aligned16(polys[i])))) { set_error("polynomial %u: null or misaligned buffer", i); return LW_ERR_BAD_ARG; }
        if (lens[i] > POLY_MAX_LEN) { set_error("polynomial %u: %zu coefficients", i, lens[i]); return LW_ERR_ALLOC; }
        *n = lens[i] > *n ? lens[i] : *n;
    }
    const uint64_t nq = *n ? *n - 1 : 0;
    if (nq > srs_len(srs)) {   // the reference panics slicing srs[..len] (kzg.rs:164-166)
        set_error("quotient of %llu coefficients is longer than the SRS (%zu points)", (unsigned long long)nq, srs_len(srs));
        return LW_ERR_LENGTH_MISMATCH;
    }
    return LW_OK;
}

// host polynomials -> one device staging block; refs point into it
static int stage_polys(Context &c, const void *const *polys, const size_t *lens, uint32_t k, std::vector<PolyRef> &refs, hipStream_t s) {
    size_t total = 0;
    for (uint32_t i = 0; i < k; i++) total += lens[i];
    if (c.host_io_a.ensure(total * 32)) return LW_ERR_ALLOC;
    refs.resize(k);
    size_t off = 0;
    for (uint32_t i = 0; i < k; i++) {
        char *d = (char *)c.host_io_a.p + off * 32;
        if (lens[i]) LW_HIP_CHECK(hipMemcpyAsync(d, polys[i], lens[i] * 32, hipMemcpyHostToDevice, s), LW_ERR_LAUNCH);
        refs[i] = PolyRef{d, (uint64_t)lens[i]};
        off += lens[i];
    }
    return LW_OK;
}

}  // namespace lw

using namespace lw;

extern "C" {

static int poly_evaluate_entry(lw_field_t field, const void *const *polys, const size_t *lens, uint32_t k, const void *points, uint32_t m,
                               void *out_values, void *hip_stream, bool device) {
    if (!poly_field_ok(field)) return LW_ERR_BAD_ARG;
    if ((k && (!polys || !lens)) || (k && m && (!points || !out_values))) { set_error("null argument"); return LW_ERR_BAD_ARG; }
    for (uint32_t i = 0; i < k; i++) {
        if (lens[i] && (!polys[i] || (device && !aligned16(polys[i])))) { set_error("polynomial %u: null or misaligned buffer", i); return LW_ERR_BAD_ARG; }
        if (lens[i] > POLY_MAX_LEN) { set_error("polynomial %u: %zu coefficients", i, lens[i]); return LW_ERR_ALLOC; }
    }
    if (k == 0 || m == 0) return LW_OK;
    Entry en(hip_stream);
    if (en.rc) return en.rc;
    Context &c = en.c;
    hipStream_t s = en.stream;
    std::vector<PolyRef> refs;
    if (device) {
        refs.resize(k);
        for (uint32_t i = 0; i < k; i++) refs[i] = PolyRef{polys[i], (uint64_t)lens[i]};
    } else {
        s = en.use_lane_stream();
        if (!s) return en.rc;
        int rc = stage_polys(c, polys, lens, k, refs, s);
        if (rc) return rc;
    }
    return field == LW_FIELD_STARK252 ? evaluate_locked<Stark252>(c, refs.data(), k, points, m, out_values, s)
                                      : evaluate_locked<Fr381>(c, refs.data(), k, points, m, out_values, s);
}
int lw_poly_evaluate(lw_field_t field, const void *const *polys, const size_t *lens, uint32_t k, const void *points, uint32_t m,
                     void *out_values) {
    return poly_evaluate_entry(field, polys, lens, k, points, m, out_values, nullptr, false);
}
int lw_poly_evaluate_device(lw_field_t field, const void *const *d_polys, const size_t *lens, uint32_t k, const void *points, uint32_t m,
                            void *out_values_host, void *hip_stream) {
    return poly_evaluate_entry(field, d_polys, lens, k, points, m, out_values_host, hip_stream, true);
}

static int ruffini_check(lw_field_t field, const void *coeffs, size_t n, const void *x, const void *out_q, bool device) {
    if (!poly_field_ok(field)) return LW_ERR_BAD_ARG;
    if (!x || (n && !coeffs) || (n > 1 && !out_q)) { set_error("null argument"); return LW_ERR_BAD_ARG; }
    if (n > POLY_MAX_LEN) { set_error("%zu coefficients", n); return LW_ERR_ALLOC; }
    if (device && n > 1) {
        if (!aligned16(coeffs) || !aligned16(out_q)) { set_error("device buffers must be 16-byte aligned"); return LW_ERR_BAD_ARG; }
        const uintptr_t a = (uintptr_t)coeffs, b = (uintptr_t)out_q;
        if (a < b + (n - 1) * 32 && b < a + n * 32) { set_error("the quotient overlaps the coefficients"); return LW_ERR_BAD_ARG; }
    }
    return LW_OK;
}
int lw_poly_ruffini_division(lw_field_t field, const void *coeffs, size_t n, const void *x, void *out_quotient, void *out_remainder_or_null) {
    int rc = ruffini_check(field, coeffs, n, x, out_quotient, false);
    if (rc) return rc;
    if (n == 0) {
        if (out_remainder_or_null) memset(out_remainder_or_null, 0, 32);
        return LW_OK;
    }
    Entry en(nullptr);
    if (en.rc) return en.rc;
    Context &c = en.c;
    hipStream_t s = en.use_lane_stream();
    if (!s) return en.rc;
    const void *polys[1] = {coeffs};
    const size_t lens[1] = {n};
    std::vector<PolyRef> refs;
    rc = stage_polys(c, polys, lens, 1, refs, s);
    if (rc) return rc;
    if (c.host_io_b.ensure((n - 1) * 32)) return LW_ERR_ALLOC;
    alignas(16) uint64_t rem[4];
    rc = field == LW_FIELD_STARK252 ? divide_locked<Stark252, false>(c, refs.data(), 1, x, nullptr, c.host_io_b.p, nullptr, rem, s)
                                    : divide_locked<Fr381, false>(c, refs.data(), 1, x, nullptr, c.host_io_b.p, nullptr, rem, s);
    if (rc) return rc;
    if (n > 1) {
        LW_HIP_CHECK(hipMemcpyAsync(out_quotient, c.host_io_b.p, (n - 1) * 32, hipMemcpyDeviceToHost, s), LW_ERR_LAUNCH);
        LW_HIP_CHECK(hipStreamSynchronize(s), LW_ERR_LAUNCH);
    }
    if (out_remainder_or_null) memcpy(out_remainder_or_null, rem, 32);
    return LW_OK;
}
int lw_poly_ruffini_division_device(lw_field_t field, const void *d_coeffs, size_t n, const void *x, void *d_out_quotient,
                                    void *out_remainder_host_or_null, void *hip_stream) {
    int rc = ruffini_check(field, d_coeffs, n, x, d_out_quotient, true);
    if (rc) return rc;
    if (n == 0) {
        if (out_remainder_host_or_null) memset(out_remainder_host_or_null, 0, 32);
        return LW_OK;
    }
    Entry en(hip_stream);
    if (en.rc) return en.rc;
    const PolyRef ref{d_coeffs, (uint64_t)n};
    return field == LW_FIELD_STARK252
               ? divide_locked<Stark252, false>(en.c, &ref, 1, x, nullptr, d_out_quotient, nullptr, out_remainder_host_or_null, en.stream)
               : divide_locked<Fr381, false>(en.c, &ref, 1, x, nullptr, d_out_quotient, nullptr, out_remainder_host_or_null, en.stream);
}

// compute_deep_composition_poly (provers/stark/src/prover.rs:643-714) over a weight matrix, see include/lw_hip.h
static int deep_entry(lw_field_t field, const void *const *polys, const size_t *lens, uint32_t k, const void *points, uint32_t m,
                      const void *weights, void *out, size_t *out_len, void *out_evals, void *hip_stream, bool device) {
    if (!poly_field_ok(field)) return LW_ERR_BAD_ARG;
    if (m == 0) { set_error("no division point"); return LW_ERR_BAD_ARG; }
    if (!points || (k && (!polys || !lens || !weights))) { set_error("null argument"); return LW_ERR_BAD_ARG; }
    uint64_t n = 0;
    for (uint32_t i = 0; i < k; i++) {
        if (lens[i] && (!polys[i] || (device && !aligned16(polys[i])))) { set_error("polynomial %u: null or misaligned buffer", i); return LW_ERR_BAD_ARG; }
        if (lens[i] > POLY_MAX_LEN) { set_error("polynomial %u: %zu coefficients", i, lens[i]); return LW_ERR_ALLOC; }
        n = lens[i] > n ? lens[i] : n;
    }
    if (n > 1) {
        if (!out) { set_error("null argument"); return LW_ERR_BAD_ARG; }
        if (device) {
            if (!aligned16(out)) { set_error("device buffers must be 16-byte aligned"); return LW_ERR_BAD_ARG; }
            const uintptr_t b = (uintptr_t)out;
            for (uint32_t i = 0; i < k; i++) {
                const uintptr_t p = (uintptr_t)polys[i];
                if (lens[i] && p < b + (n - 1) * 32 && b < p + lens[i] * 32) { set_error("the output overlaps polynomial %u", i); return LW_ERR_BAD_ARG; }
            }
        }
    }
    const char *W = (const char *)weights;
    if (n <= 1) {   // constants and empty polynomials: an empty result; the values are the constants themselves
        if (out_len) *out_len = 0;
        if (!out_evals) return LW_OK;
        memset(out_evals, 0, (size_t)k * m * 32);
        if (n == 0) return LW_OK;
        std::vector<uint64_t> c0((size_t)k * 4, 0);
        if (device) {
            Entry en(hip_stream);
            if (en.rc) return en.rc;
            for (uint32_t i = 0; i < k; i++)
                if (lens[i]) LW_HIP_CHECK(hipMemcpyAsync(&c0[(size_t)i * 4], polys[i], 32, hipMemcpyDeviceToHost, en.stream), LW_ERR_LAUNCH);
            LW_HIP_CHECK(hipStreamSynchronize(en.stream), LW_ERR_LAUNCH);
        } else {
            for (uint32_t i = 0; i < k; i++)
                if (lens[i]) memcpy(&c0[(size_t)i * 4], polys[i], 32);
        }
        for (uint32_t i = 0; i < k; i++)
            for (uint32_t j = 0; j < m; j++)
                if (!elem_is_zero(W + ((size_t)i * m + j) * 32)) memcpy((char *)out_evals + ((size_t)i * m + j) * 32, &c0[(size_t)i * 4], 32);
        return LW_OK;
    }
    Entry en(hip_stream);
    if (en.rc) return en.rc;
    Context &c = en.c;
    hipStream_t s = en.stream;
    std::vector<PolyRef> refs;
    void *d_out = out;
    if (device) {
        refs.resize(k);
        for (uint32_t i = 0; i < k; i++) refs[i] = PolyRef{polys[i], (uint64_t)lens[i]};
    } else {
        s = en.use_lane_stream();
        if (!s) return en.rc;
        int rc = stage_polys(c, polys, lens, k, refs, s);
        if (rc) return rc;
        if (c.host_io_b.ensure((n - 1) * 32)) return LW_ERR_ALLOC;
        d_out = c.host_io_b.p;
    }
    int rc = field == LW_FIELD_STARK252 ? deep_locked<Stark252>(c, refs.data(), k, points, m, weights, d_out, out_len, out_evals, s)
                                        : deep_locked<Fr381>(c, refs.data(), k, points, m, weights, d_out, out_len, out_evals, s);
    if (rc || device) return rc;
    LW_HIP_CHECK(hipMemcpyAsync(out, d_out, (n - 1) * 32, hipMemcpyDeviceToHost, s), LW_ERR_LAUNCH);
    LW_HIP_CHECK(hipStreamSynchronize(s), LW_ERR_LAUNCH);
    return LW_OK;
}
int lw_stark_deep_composition(lw_field_t field, const void *const *polys, const size_t *lens, uint32_t k, const void *points, uint32_t m,
                              const void *weights, void *out_coeffs, size_t *out_len_or_null, void *out_evals_or_null) {
    return deep_entry(field, polys, lens, k, points, m, weights, out_coeffs, out_len_or_null, out_evals_or_null, nullptr, false);
}
int lw_stark_deep_composition_device(lw_field_t field, const void *const *d_polys, const size_t *lens, uint32_t k, const void *points,
                                     uint32_t m, const void *weights, void *d_out_coeffs, size_t *out_len_or_null,
                                     void *out_evals_host_or_null, void *hip_stream) {
    return deep_entry(field, d_polys, lens, k, points, m, weights, d_out_coeffs, out_len_or_null, out_evals_host_or_null, hip_stream, true);
}

static int kzg_entry(const lw_srs_t *srs, const void *const *polys, const size_t *lens, uint32_t k, const uint64_t *x, const uint64_t *ups,
                     void *out_proof, uint64_t *out_evals, uint64_t *out_eval, void *hip_stream, bool device) {
    uint64_t n = 0;
    int rc = kzg_check(srs, polys, lens, k, x, ups, out_proof, device, &n);
    if (rc) return rc;
    Entry en(hip_stream);
    if (en.rc) return en.rc;
    Context &c = en.c;
    hipStream_t s = en.stream;
    std::vector<PolyRef> refs;
    if (device) {
        refs.resize(k);
        for (uint32_t i = 0; i < k; i++) refs[i] = PolyRef{polys[i], (uint64_t)lens[i]};
    } else {
        s = en.use_lane_stream();
        if (!s) return en.rc;
        rc = stage_polys(c, polys, lens, k, refs, s);
        if (rc) return rc;
    }
    return kzg_open_locked(c, srs, refs.data(), k, x, ups, out_proof, out_evals, out_eval, s);
}
int lw_kzg_open(const lw_srs_t *srs, const uint64_t *coeffs, size_t n, const uint64_t *x, void *out_proof, uint64_t *out_eval_or_null) {
    const void *polys[1] = {coeffs};
    return kzg_entry(srs, polys, &n, 1, x, nullptr, out_proof, nullptr, out_eval_or_null, nullptr, false);
}
int lw_kzg_open_device(const lw_srs_t *srs, const uint64_t *d_coeffs, size_t n, const uint64_t *x, void *out_proof_host,
                       uint64_t *out_eval_host_or_null, void *hip_stream) {
    const void *polys[1] = {d_coeffs};
    return kzg_entry(srs, polys, &n, 1, x, nullptr, out_proof_host, nullptr, out_eval_host_or_null, hip_stream, true);
}
int lw_kzg_open_batch(const lw_srs_t *srs, const uint64_t *const *polys, const size_t *lens, uint32_t k, const uint64_t *x,
                      const uint64_t *upsilon, void *out_proof, uint64_t *out_evals_or_null) {
    return kzg_entry(srs, (const void *const *)polys, lens, k, x, upsilon, out_proof, out_evals_or_null, nullptr, nullptr, false);
}
int lw_kzg_open_batch_device(const lw_srs_t *srs, const uint64_t *const *d_polys, const size_t *lens, uint32_t k, const uint64_t *x,
                             const uint64_t *upsilon, void *out_proof_host, uint64_t *out_evals_host_or_null, void *hip_stream) {
    return kzg_entry(srs, (const void *const *)d_polys, lens, k, x, upsilon, out_proof_host, out_evals_host_or_null, nullptr, hip_stream, true);
}

}  // extern "C"
