// A rank-one constraint system resident on the device: three sparse matrices A, B, C over Stark252 or BLS12-381 Fr, and
// the two products the provers take of them.  Elements are those of multilinear.hip (stored Montgomery residues).
//
//   matvec     out_M[i] = sum_j M[i,j] z[j], i < n_rows, for M = A, B, C; zero for n_rows <= i < n_out.
//   bind_rows  out[j] = sum_i e[i] (c_A A[i,j] + c_B B[i,j] + c_C C[i,j]), j < n_cols; zero for n_cols <= j < n_out.
//
// Both are one gather over index lists: matvec over the rows of the three matrices (CSR as the caller gave it), bind_rows
// over their columns (the transposed index, built once by lw_r1cs_create with the rows of a column in ascending order).
// A list entry is one u32: the gathered index in the low 30 bits (n_rows, n_cols <= 2^30) and the class of its value in
// the top two: one, minus one or general.  Only a general entry reads its 32-byte value and costs a product.
//
// Work split.  The median list has one or two entries, so a work-item of r1cs_lists_kernel takes one output index and
// walks the lists of all three matrices there: 64 outputs per wave, nobody idles on a short list.  A wave then runs as
// long as its longest lane, so a list of more than R1CS_SPLIT entries is left out of that kernel: lw_r1cs_create cuts it
// into pieces of R1CS_SPLIT entries, r1cs_pieces_kernel sums one piece per work-item into the partials (the loads of
// R1CS_BATCH entries in flight at a time), and r1cs_long_kernel adds the partials of every output that has a long list
// and finishes it: one work-item per output with at most R1CS_FEW pieces per matrix (the widest gates of a circuit), one
// block per output with more (the constant column), every work-item its own stride of the pieces in ascending order and
// then the block's tree.  No atomics; every stored value is a canonical residue, so the order of the additions does not
// show in a result.
//
// Accumulation.  Stark252 (p < 2^252, 2^256 / p = 31.99..): a term is z[j] (< p), p - z[j] (<= p) or the lazy product
// value * z[j] (< 2p, the value is canonical: checked by lw_r1cs_create), so R1CS_TERMS = 15 terms sum to less than
// 30p < 2^256 in eight limbs without a reduction; 16 terms could reach 32p > 2^256.  A list is summed in groups of
// R1CS_TERMS terms, each group reduced fully once (fe_reduce_full) and added to the canonical running sum.  Fr381 has no
// headroom above 2p (2^256 / p = 2.2): there two general terms share one reduction (fe_dot, KSUM = 2 is its bound) and
// the classes one and minus one are a canonical add and subtract.
#include <algorithm>
#include "multilinear.cuh"

namespace lw {

constexpr int R1CS_THREADS = 256;
constexpr uint32_t R1CS_TERMS = 15;                 // unreduced terms of at most 2p each that fit 2^256 over Stark252
constexpr uint32_t R1CS_SPLIT = 2 * R1CS_TERMS;     // entries of the longest list one work-item walks; also a piece's length
constexpr int R1CS_BATCH = 5;                       // entries of a piece whose loads are issued together
constexpr uint32_t R1CS_FEW = 8;                    // a long output with at most this many pieces per matrix is added up by one work-item
constexpr uint32_t R1CS_INDEX_BITS = 30;
constexpr uint32_t R1CS_INDEX_MASK = (1u << R1CS_INDEX_BITS) - 1;
enum : uint32_t { R1CS_GENERAL = 0, R1CS_ONE = 1, R1CS_MINUS_ONE = 2 };
static_assert(2ull * R1CS_TERMS * ((uint64_t)Stark252::p(7) + 1) <= (1ull << 32), "R1CS_TERMS terms below 2p must fit 2^256");

struct R1csPiece { uint32_t m, first, end, pad; };                 // entries [first, end) of matrix m's lists
struct R1csLong { uint32_t index, first[3], count[3], pad; };      // an output index and, per matrix, its pieces (count 0: none)

struct R1csLists {   // one direction of the three matrices: device pointers
    const uint32_t *ptr[3];     // n_lists + 1 offsets
    const uint32_t *ent[3];     // index | class << 30
    const char *val[3];         // 32 bytes per entry
    const R1csPiece *pieces;
    const R1csLong *longs;
    uint32_t n_lists, n_pieces, n_longs, n_few;   // longs[0 .. n_few): at most R1CS_FEW pieces per matrix
};

template <class F>
struct R1csArgs {
    R1csLists l;
    const char *x;              // the gathered vector: z (matvec) or e (bind_rows)
    char *out[3];               // matvec: Az, Bz, Cz, each or null; bind_rows: out[0]
    char *partials;             // n_pieces elements
    uint64_t n_out;
    Fe<F> coeff[3];             // bind_rows only
};

// sum over entries [k, end) of value * x[index], canonical.  The entries are taken U at a time: the U entry words first,
// then the U gathered elements and the values of the general ones, then the arithmetic, so that the loads of a batch are in
// flight together.  U = 1 for the short lists of r1cs_lists_kernel (a batch would mostly be empty slots), U = R1CS_BATCH
// for the pieces, which are full.  A slot past the end counts as the class one with the element zero.
template <class F, int U>
__device__ __forceinline__ Fe<F> r1cs_sum(const uint32_t *ent, const char *val, const char *x, uint32_t k, uint32_t end) {
    static_assert(R1CS_TERMS % U == 0, "a group of R1CS_TERMS terms is a whole number of batches");
    Fe<F> acc = Fe<F>::zero();
    Fe<F> raw = Fe<F>::zero();   // Stark252: < 2p per term added, reduced before a batch could make it more than R1CS_TERMS terms
    uint32_t in_raw = 0;
    Fe<F> pv = Fe<F>::zero(), px = Fe<F>::zero();   // Fr381: a general term waiting for a second one to share its reduction
    bool have = false;
#pragma unroll 1
    for (; k < end; k += U) {
        uint32_t e[U];
        Fe<F> xv[U], v[U];
#pragma unroll
        for (int u = 0; u < U; u++) e[u] = k + u < end ? ent[k + u] : (R1CS_ONE << R1CS_INDEX_BITS);
#pragma unroll
        for (int u = 0; u < U; u++) {
            xv[u] = k + u < end ? fe_load<F>(x + (uint64_t)(e[u] & R1CS_INDEX_MASK) * 32) : Fe<F>::zero();
            v[u] = (e[u] >> R1CS_INDEX_BITS) == R1CS_GENERAL ? fe_load<F>(val + (uint64_t)(k + u) * 32) : Fe<F>::zero();
        }
#pragma unroll
        for (int u = 0; u < U; u++) {
            const uint32_t cls = e[u] >> R1CS_INDEX_BITS;
            if constexpr (F::LAZY) {
                Fe<F> t;
                if (cls == R1CS_ONE) t = xv[u];
                else if (cls == R1CS_MINUS_ONE) t = fe_neg_raw<F>(xv[u]);
                else t = fe_mul_lazy<F>(v[u], xv[u]);
                raw = fe_add_raw<F>(raw, t);
            } else if (cls == R1CS_ONE) {
                acc = fe_add<F>(acc, xv[u]);
            } else if (cls == R1CS_MINUS_ONE) {
                acc = fe_sub<F>(acc, xv[u]);
            } else if (have) {
                const Fe<F> *const pa[2] = {&pv, &v[u]}, *const pb[2] = {&px, &xv[u]};
                acc = fe_add<F>(acc, fe_dot<F, 2>(pa, pb));
                have = false;
            } else {
                pv = v[u];
                px = xv[u];
                have = true;
            }
        }
        if constexpr (F::LAZY) {
            in_raw += U;
            if (in_raw == R1CS_TERMS) {
                acc = fe_add<F>(acc, fe_reduce_full(raw));
                raw = Fe<F>::zero();
                in_raw = 0;
            }
        }
    }
    if constexpr (F::LAZY) {
        if (in_raw) acc = fe_add<F>(acc, fe_reduce_full(raw));
    } else {
        if (have) acc = fe_add<F>(acc, fe_mul<F>(pv, px));
    }
    return acc;
}

// Work-item i: output index i of every matrix.  Lists of more than R1CS_SPLIT entries are left to the two kernels below:
// matvec does not write their outputs here, bind_rows writes the sum over the other lists and r1cs_long_kernel adds to it.
template <class F, bool COMBINE>
__global__ __launch_bounds__(R1CS_THREADS) void r1cs_lists_kernel(const R1csArgs<F> a) {
    const uint64_t i = (uint64_t)blockIdx.x * R1CS_THREADS + threadIdx.x;
    if (i >= a.n_out) return;
    const bool inside = i < a.l.n_lists;
    Fe<F> comb = Fe<F>::zero();
#pragma unroll
    for (int m = 0; m < 3; m++) {
        if (!COMBINE && !a.out[m]) continue;   // uniform
        uint32_t b = 0, e = 0;
        if (inside) {
            b = a.l.ptr[m][i];
            e = a.l.ptr[m][i + 1];
        }
        const bool is_long = e - b > R1CS_SPLIT;
        Fe<F> s = Fe<F>::zero();
        if (e > b && !is_long) s = r1cs_sum<F, 1>(a.l.ent[m], a.l.val[m], a.x, b, e);
        if (COMBINE) {
            if (e > b && !is_long) comb = fe_add<F>(comb, fe_mul<F>(a.coeff[m], s));
        } else if (!is_long) {
            fe_store<F>(a.out[m] + i * 32, s);
        }
    }
    if (COMBINE) fe_store<F>(a.out[0] + i * 32, comb);
}

template <class F, bool COMBINE>
__global__ __launch_bounds__(R1CS_THREADS) void r1cs_pieces_kernel(const R1csArgs<F> a) {
    const uint32_t p = blockIdx.x * R1CS_THREADS + threadIdx.x;
    if (p >= a.l.n_pieces) return;
    const R1csPiece pc = a.l.pieces[p];
    const uint32_t m = pc.m;
    const uint32_t *ent = m == 0 ? a.l.ent[0] : m == 1 ? a.l.ent[1] : a.l.ent[2];
    const char *val = m == 0 ? a.l.val[0] : m == 1 ? a.l.val[1] : a.l.val[2];
    if (!COMBINE) {
        const char *o = m == 0 ? a.out[0] : m == 1 ? a.out[1] : a.out[2];
        if (!o) return;   // this product was not asked for
    }
    fe_store<F>(a.partials + (uint64_t)p * 32, r1cs_sum<F, R1CS_BATCH>(ent, val, a.x, pc.first, pc.end));
}

// The outputs that have a long list; per matrix with pieces there, the sum of their partials.  longs[0 .. n_few) have at
// most R1CS_FEW pieces per matrix (a row of the circuit's widest gate): one work-item each, in the leading blocks.  Every
// later block takes one of the others (a column that half the rows name): each work-item adds its own stride of the
// partials, four loads in flight, then the block's tree.
template <class F, bool COMBINE>
__global__ __launch_bounds__(R1CS_THREADS) void r1cs_long_kernel(const R1csArgs<F> a) {
    __shared__ Fe<F> lds[R1CS_THREADS];
    const uint32_t few_blocks = (a.l.n_few + R1CS_THREADS - 1) / R1CS_THREADS;
    const bool few = blockIdx.x < few_blocks;   // the same in every work-item of the block
    const uint32_t which = few ? blockIdx.x * R1CS_THREADS + threadIdx.x : a.l.n_few + (blockIdx.x - few_blocks);
    if (few && which >= a.l.n_few) return;
    const R1csLong L = a.l.longs[which];
    const bool writer = few || threadIdx.x == 0;
    Fe<F> comb = Fe<F>::zero();
#pragma unroll
    for (int m = 0; m < 3; m++) {
        if (!COMBINE && !a.out[m]) continue;   // uniform
        Fe<F> acc = Fe<F>::zero();
        const char *part = a.partials + (uint64_t)L.first[m] * 32;
        if (few) {
            if (L.count[m] == 0) continue;
#pragma unroll 1
            for (uint32_t p = 0; p < L.count[m]; p++) acc = fe_add<F>(acc, fe_load<F>(part + (uint64_t)p * 32));
        } else {
            if (L.count[m] == 0) continue;   // the same in every work-item of the block: one output a block
            uint32_t p = threadIdx.x;
#pragma unroll 1
            for (; p + 3 * R1CS_THREADS < L.count[m]; p += 4 * R1CS_THREADS) {
                const Fe<F> t0 = fe_load<F>(part + (uint64_t)p * 32), t1 = fe_load<F>(part + (uint64_t)(p + R1CS_THREADS) * 32);
                const Fe<F> t2 = fe_load<F>(part + (uint64_t)(p + 2 * R1CS_THREADS) * 32);
                const Fe<F> t3 = fe_load<F>(part + (uint64_t)(p + 3 * R1CS_THREADS) * 32);
                acc = fe_add<F>(fe_add<F>(acc, fe_add<F>(t0, t1)), fe_add<F>(t2, t3));
            }
#pragma unroll 1
            for (; p < L.count[m]; p += R1CS_THREADS) acc = fe_add<F>(acc, fe_load<F>(part + (uint64_t)p * 32));
            acc = ml_block_sum<F>(acc, lds);
        }
        if (writer) {
            if (COMBINE) comb = fe_add<F>(comb, fe_mul<F>(a.coeff[m], acc));
            else fe_store<F>(a.out[m] + (uint64_t)L.index * 32, acc);
        }
    }
    if (COMBINE && writer) {
        char *o = a.out[0] + (uint64_t)L.index * 32;
        fe_store<F>(o, fe_add<F>(fe_load<F>(o), comb));
    }
}

// *best = min(*best, smallest i < n with az[i] * bz[i] != cz[i]): one atomicMin per block that holds a broken row
template <class F>
__global__ __launch_bounds__(R1CS_THREADS) void r1cs_check_kernel(const char *az, const char *bz, const char *cz, uint32_t n,
                                                                  unsigned long long *best) {
    __shared__ unsigned int block_min;
    if (threadIdx.x == 0) block_min = 0xffffffffu;
    __syncthreads();
    const uint32_t i = blockIdx.x * R1CS_THREADS + threadIdx.x;
    if (i < n) {
        const Fe<F> ab = fe_mul<F>(fe_load<F>(az + (uint64_t)i * 32), fe_load<F>(bz + (uint64_t)i * 32));
        if (ab != fe_load<F>(cz + (uint64_t)i * 32)) atomicMin(&block_min, i);   // LDS
    }
    __syncthreads();
    if (threadIdx.x == 0 && block_min != 0xffffffffu) atomicMin(best, (unsigned long long)block_min);
}

}  // namespace lw

// ---- the handle ----
struct lw_r1cs {
    lw_field_t field;
    uint32_t n_rows, n_cols;
    lw::DeviceBuf image;      // every array below
    lw::R1csLists rows, cols; // matvec walks rows, bind_rows walks cols
};

namespace lw {

static uint32_t r1cs_blocks(uint64_t n) { return (uint32_t)((n + R1CS_THREADS - 1) / R1CS_THREADS); }

template <class F, bool COMBINE>
static int r1cs_run(Context &c, const R1csLists &l, const void *d_x, void *const (&d_out)[3], const void *coeffs3, uint64_t n_out,
                    hipStream_t s) {
    R1csArgs<F> a;
    memset(&a, 0, sizeof(a));
    a.l = l;
    a.x = (const char *)d_x;
    for (int m = 0; m < 3; m++) a.out[m] = (char *)d_out[m];
    a.n_out = n_out;
    if (COMBINE)
        for (int m = 0; m < 3; m++) a.coeff[m] = ml_load<F>((const char *)coeffs3 + (size_t)m * 32);
    if (l.n_pieces) {   // sized by lw_r1cs_create on its lane; another lane grows once
        if (c.poly_ws.ensure(256 + (size_t)l.n_pieces * 32)) return LW_ERR_ALLOC;
        a.partials = (char *)c.poly_ws.p + 256;
    }
    hipEvent_t pe = c.prof_begin(s);
    hipLaunchKernelGGL((r1cs_lists_kernel<F, COMBINE>), dim3(r1cs_blocks(n_out)), dim3(R1CS_THREADS), 0, s, a);
    c.prof_end(COMBINE ? "r1cs_lists_kernel(bind)" : "r1cs_lists_kernel", pe, s);
    if (l.n_pieces) {
        pe = c.prof_begin(s);
        hipLaunchKernelGGL((r1cs_pieces_kernel<F, COMBINE>), dim3(r1cs_blocks(l.n_pieces)), dim3(R1CS_THREADS), 0, s, a);
        c.prof_end("r1cs_pieces_kernel", pe, s);
        pe = c.prof_begin(s);
        hipLaunchKernelGGL((r1cs_long_kernel<F, COMBINE>), dim3(r1cs_blocks(l.n_few) + (l.n_longs - l.n_few)), dim3(R1CS_THREADS), 0, s, a);
        c.prof_end("r1cs_long_kernel", pe, s);
    }
    LW_HIP_CHECK(hipGetLastError(), LW_ERR_LAUNCH);
    return LW_OK;
}

lw_field_t r1cs_field(const lw_r1cs_t *h) { return h->field; }
uint32_t r1cs_rows(const lw_r1cs_t *h) { return h->n_rows; }
uint32_t r1cs_cols(const lw_r1cs_t *h) { return h->n_cols; }

int r1cs_matvec_locked(Context &c, const lw_r1cs_t *h, const void *d_z, size_t n_out, void *const (&d_out)[3], hipStream_t s) {
    if (!d_out[0] && !d_out[1] && !d_out[2]) return LW_OK;
    return h->field == LW_FIELD_STARK252 ? r1cs_run<Stark252, false>(c, h->rows, d_z, d_out, nullptr, n_out, s)
                                         : r1cs_run<Fr381, false>(c, h->rows, d_z, d_out, nullptr, n_out, s);
}

static int r1cs_bind_locked(Context &c, const lw_r1cs_t *h, const void *d_e, const void *coeffs3, size_t n_out, void *d_out, hipStream_t s) {
    void *const out[3] = {d_out, nullptr, nullptr};
    return h->field == LW_FIELD_STARK252 ? r1cs_run<Stark252, true>(c, h->cols, d_e, out, coeffs3, n_out, s)
                                         : r1cs_run<Fr381, true>(c, h->cols, d_e, out, coeffs3, n_out, s);
}

// Az, Bz, Cz into the lane's tables, then the smallest broken row -> *out_row (-1: none).  Synchronises.
static int r1cs_check_locked(Context &c, const lw_r1cs_t *h, const void *d_z, int64_t *out_row, hipStream_t s) {
    const size_t tb = ml_round256((size_t)h->n_rows * 32);
    if (c.poly_q.ensure(3 * tb) || c.poly_ws.ensure(256)) return LW_ERR_ALLOC;
    char *t = (char *)c.poly_q.p;
    void *const tabs[3] = {t, t + tb, t + 2 * tb};
    int rc = r1cs_matvec_locked(c, h, d_z, h->n_rows, tabs, s);
    if (rc) return rc;
    unsigned long long *best = (unsigned long long *)c.poly_ws.p;   // the partials start 256 bytes in
    LW_HIP_CHECK(hipMemsetAsync(best, 0xff, 8, s), LW_ERR_LAUNCH);
    hipEvent_t pe = c.prof_begin(s);
    if (h->field == LW_FIELD_STARK252)
        hipLaunchKernelGGL((r1cs_check_kernel<Stark252>), dim3(r1cs_blocks(h->n_rows)), dim3(R1CS_THREADS), 0, s, t, t + tb, t + 2 * tb,
                           h->n_rows, best);
    else
        hipLaunchKernelGGL((r1cs_check_kernel<Fr381>), dim3(r1cs_blocks(h->n_rows)), dim3(R1CS_THREADS), 0, s, t, t + tb, t + 2 * tb,
                           h->n_rows, best);
    c.prof_end("r1cs_check_kernel", pe, s);
    LW_HIP_CHECK(hipGetLastError(), LW_ERR_LAUNCH);
    uint64_t v = 0;
    rc = ml_result(c, best, 8, &v, s);
    if (rc) return rc;
    *out_row = v == ~0ull ? -1 : (int64_t)v;
    return LW_OK;
}

// ---- lw_r1cs_create: checks, classes, the transposed index, the plan of the long lists ----
struct R1csHostSide {   // one direction, host arrays
    std::vector<uint32_t> ptr[3], ent[3];
    std::vector<uint64_t> val[3];   // 4 words per entry
    std::vector<R1csPiece> pieces;
    std::vector<R1csLong> longs;    // those with at most R1CS_FEW pieces per matrix first
    uint32_t n_few = 0;
};

static void r1cs_plan(R1csHostSide &hs, uint32_t n_lists) {
    for (uint32_t i = 0; i < n_lists; i++) {
        R1csLong L = {i, {0, 0, 0}, {0, 0, 0}, 0};
        bool any = false;
        for (int m = 0; m < 3; m++) {
            const uint32_t b = hs.ptr[m][i], e = hs.ptr[m][i + 1];
            if (e - b <= R1CS_SPLIT) continue;
            any = true;
            L.first[m] = (uint32_t)hs.pieces.size();
            for (uint32_t k = b; k < e; k += R1CS_SPLIT) hs.pieces.push_back({(uint32_t)m, k, e - k > R1CS_SPLIT ? k + R1CS_SPLIT : e, 0});
            L.count[m] = (uint32_t)hs.pieces.size() - L.first[m];
        }
        if (any) hs.longs.push_back(L);
    }
    auto is_few = [](const R1csLong &L) { return L.count[0] <= R1CS_FEW && L.count[1] <= R1CS_FEW && L.count[2] <= R1CS_FEW; };
    hs.n_few = (uint32_t)(std::stable_partition(hs.longs.begin(), hs.longs.end(), is_few) - hs.longs.begin());
}

template <class F>
static int r1cs_build_host(uint32_t n_rows, uint32_t n_cols, const uint32_t *const row_ptr[3], const uint32_t *const col_idx[3],
                           const void *const values[3], R1csHostSide &rs, R1csHostSide &cs) {
    const Fe<F> one = Fe<F>::one(), minus_one = fe_neg<F>(one);
    uint32_t pw[F::N];
    for (int k = 0; k < F::N; k++) pw[k] = F::p(k);
    for (int m = 0; m < 3; m++) {
        const uint32_t *rp = row_ptr[m];
        if (rp[0] != 0) { set_error("matrix %d: row_ptr[0] = %u, not 0", m, rp[0]); return LW_ERR_BAD_ARG; }
        for (uint32_t i = 0; i < n_rows; i++)
            if (rp[i + 1] < rp[i]) { set_error("matrix %d: row_ptr decreases at row %u", m, i); return LW_ERR_BAD_ARG; }
        const uint32_t nnz = rp[n_rows];
        if (nnz && (!col_idx[m] || !values[m])) { set_error("matrix %d: %u entries but a null array", m, nnz); return LW_ERR_BAD_ARG; }
        rs.ptr[m].assign(rp, rp + n_rows + 1);
        rs.ent[m].resize(nnz);
        rs.val[m].resize((size_t)nnz * 4);
        if (nnz) memcpy(rs.val[m].data(), values[m], (size_t)nnz * 32);
        std::vector<uint32_t> &cp = cs.ptr[m];
        cp.assign((size_t)n_cols + 1, 0);
        for (uint32_t k = 0; k < nnz; k++) {
            const uint32_t j = col_idx[m][k];
            if (j >= n_cols) { set_error("matrix %d: entry %u names column %u of %u", m, k, j, n_cols); return LW_ERR_BAD_ARG; }
            const Fe<F> v = ml_load<F>((const char *)values[m] + (size_t)k * 32);
            uint32_t d[F::N];
            if (limbs_sub<F::N>(d, v.v, pw) == 0) { set_error("matrix %d: the value of entry %u is not below the modulus", m, k); return LW_ERR_BAD_ARG; }
            const uint32_t cls = v == one ? R1CS_ONE : v == minus_one ? R1CS_MINUS_ONE : R1CS_GENERAL;
            rs.ent[m][k] = j | (cls << R1CS_INDEX_BITS);
            cp[j + 1]++;
        }
        for (uint32_t j = 0; j < n_cols; j++) cp[j + 1] += cp[j];
        // the transposed lists: rows in ascending order inside a column (a stable counting sort by column)
        cs.ent[m].resize(nnz);
        cs.val[m].resize((size_t)nnz * 4);
        std::vector<uint32_t> cursor(cp.begin(), cp.end() - 1);
        for (uint32_t i = 0; i < n_rows; i++)
            for (uint32_t k = rp[i]; k < rp[i + 1]; k++) {
                const uint32_t e = rs.ent[m][k], pos = cursor[e & R1CS_INDEX_MASK]++;
                cs.ent[m][pos] = i | (e & ~R1CS_INDEX_MASK);
                memcpy(&cs.val[m][(size_t)pos * 4], &rs.val[m][(size_t)k * 4], 32);
            }
    }
    r1cs_plan(rs, n_rows);
    r1cs_plan(cs, n_cols);
    return LW_OK;
}

static size_t r1cs_side_bytes(const R1csHostSide &hs) {
    size_t b = 0;
    for (int m = 0; m < 3; m++)
        b += ml_round256(hs.ptr[m].size() * 4) + ml_round256(hs.ent[m].size() * 4) + ml_round256(hs.val[m].size() * 8);
    return b + ml_round256(hs.pieces.size() * sizeof(R1csPiece)) + ml_round256(hs.longs.size() * sizeof(R1csLong));
}

// host arrays -> the image at `at` (advanced), pointers into l
static int r1cs_upload_side(const R1csHostSide &hs, uint32_t n_lists, char *&at, R1csLists &l, hipStream_t s) {
    auto put = [&](const void *src, size_t bytes, const void **dst) -> int {
        *dst = at;
        if (bytes) LW_HIP_CHECK(hipMemcpyAsync(at, src, bytes, hipMemcpyHostToDevice, s), LW_ERR_LAUNCH);
        at += ml_round256(bytes);
        return LW_OK;
    };
    int rc = LW_OK;
    for (int m = 0; m < 3 && !rc; m++) {
        rc = put(hs.ptr[m].data(), hs.ptr[m].size() * 4, (const void **)&l.ptr[m]);
        if (!rc) rc = put(hs.ent[m].data(), hs.ent[m].size() * 4, (const void **)&l.ent[m]);
        if (!rc) rc = put(hs.val[m].data(), hs.val[m].size() * 8, (const void **)&l.val[m]);
    }
    if (!rc) rc = put(hs.pieces.data(), hs.pieces.size() * sizeof(R1csPiece), (const void **)&l.pieces);
    if (!rc) rc = put(hs.longs.data(), hs.longs.size() * sizeof(R1csLong), (const void **)&l.longs);
    l.n_lists = n_lists;
    l.n_pieces = (uint32_t)hs.pieces.size();
    l.n_longs = (uint32_t)hs.longs.size();
    l.n_few = hs.n_few;
    return rc;
}

static int r1cs_null() { set_error("null argument"); return LW_ERR_BAD_ARG; }
static int r1cs_misaligned() { set_error("device buffers must be 16-byte aligned"); return LW_ERR_BAD_ARG; }
constexpr size_t R1CS_MAX_OUT = (size_t)1 << 34;

}  // namespace lw

using namespace lw;

extern "C" {

uint32_t lw_r1cs_split_length(void) { return R1CS_SPLIT; }
uint32_t lw_r1cs_lazy_terms(void) { return R1CS_TERMS; }

int lw_r1cs_create(lw_field_t field, uint32_t n_rows, uint32_t n_cols, const uint32_t *const row_ptr[3], const uint32_t *const col_idx[3],
                   const void *const values[3], lw_r1cs_t **out) {
    if (!ml_field_ok(field)) return LW_ERR_BAD_ARG;
    if (!row_ptr || !col_idx || !values || !out || !row_ptr[0] || !row_ptr[1] || !row_ptr[2]) return r1cs_null();
    if (n_rows == 0 || n_cols == 0 || n_rows > (1u << R1CS_INDEX_BITS) || n_cols > (1u << R1CS_INDEX_BITS)) {
        set_error("%u rows, %u columns: each from 1 to 2^%u", n_rows, n_cols, R1CS_INDEX_BITS);
        return LW_ERR_BAD_ARG;
    }
    R1csHostSide rs, cs;
    int rc = field == LW_FIELD_STARK252 ? r1cs_build_host<Stark252>(n_rows, n_cols, row_ptr, col_idx, values, rs, cs)
                                        : r1cs_build_host<Fr381>(n_rows, n_cols, row_ptr, col_idx, values, rs, cs);
    if (rc) return rc;
    lw_r1cs *h = new (std::nothrow) lw_r1cs{};
    if (!h) return LW_ERR_ALLOC;
    h->field = field;
    h->n_rows = n_rows;
    h->n_cols = n_cols;
    {
        Entry en(nullptr);
        rc = en.rc;
        hipStream_t s = rc ? nullptr : en.use_lane_stream();
        if (rc == LW_OK && !s) rc = en.rc;
        if (rc == LW_OK && h->image.ensure(r1cs_side_bytes(rs) + r1cs_side_bytes(cs))) rc = LW_ERR_ALLOC;
        if (rc == LW_OK) {
            char *at = (char *)h->image.p;
            rc = r1cs_upload_side(rs, n_rows, at, h->rows, s);
            if (rc == LW_OK) rc = r1cs_upload_side(cs, n_cols, at, h->cols, s);
            // the partials of the longer plan, on this lane, so that matvec and bind_rows never grow them.  (They live with
            // the lane, not the handle: the library already orders a lane's buffers across streams, and two lanes may run
            // the same handle at once.)
            const size_t np = rs.pieces.size() > cs.pieces.size() ? rs.pieces.size() : cs.pieces.size();
            if (rc == LW_OK && en.c.poly_ws.ensure(256 + np * 32)) rc = LW_ERR_ALLOC;
            if (rc == LW_OK && hipStreamSynchronize(s) != hipSuccess) {   // the host arrays go away with this scope
                set_error("upload of the constraint system failed");
                rc = LW_ERR_LAUNCH;
            }
        }
        if (rc && en.rc == LW_OK) h->image.release();
    }
    if (rc) {
        delete h;
        return rc;
    }
    *out = h;
    return LW_OK;
}

int lw_r1cs_destroy(lw_r1cs_t *r1cs) {
    if (!r1cs) return LW_OK;
    Entry en(nullptr);   // binds the context's device for the hipFree
    r1cs->image.release();
    delete r1cs;
    return LW_OK;
}

static int matvec_entry(const lw_r1cs_t *h, const void *z, size_t n_out, void *az, void *bz, void *cz, void *hip_stream, bool device) {
    if (!h || !z) return r1cs_null();
    if (n_out < h->n_rows || n_out > R1CS_MAX_OUT) { set_error("n_out = %zu: from the %u rows to 2^34", n_out, h->n_rows); return LW_ERR_BAD_ARG; }
    void *outs[3] = {az, bz, cz};
    const size_t zb = (size_t)h->n_cols * 32, ob = n_out * 32;
    if (device && !ml_aligned16(z)) return r1cs_misaligned();
    for (int m = 0; m < 3; m++) {
        if (!outs[m]) continue;
        if (device && !ml_aligned16(outs[m])) return r1cs_misaligned();
        if (ml_overlap(outs[m], ob, z, zb)) { set_error("output %d overlaps z", m); return LW_ERR_BAD_ARG; }
        for (int k = 0; k < m; k++)
            if (outs[k] && ml_overlap(outs[m], ob, outs[k], ob)) { set_error("outputs %d and %d overlap", k, m); return LW_ERR_BAD_ARG; }
    }
    Entry en(hip_stream);
    if (en.rc) return en.rc;
    Context &c = en.c;
    if (device) {
        void *const d[3] = {az, bz, cz};
        return r1cs_matvec_locked(c, h, z, n_out, d, en.stream);
    }
    hipStream_t s = en.use_lane_stream();
    if (!s) return en.rc;
    if (c.host_io_b.ensure(3 * ob)) return LW_ERR_ALLOC;   // both buffers before any copy from caller memory
    int rc = ml_upload(c.host_io_a, z, zb, s);
    if (rc) return rc;
    char *o = (char *)c.host_io_b.p;
    void *const d[3] = {az ? o : nullptr, bz ? o + ob : nullptr, cz ? o + 2 * ob : nullptr};
    rc = r1cs_matvec_locked(c, h, c.host_io_a.p, n_out, d, s);
    return rc ? rc : ml_download_each(outs, d, 3, ob, s);
}
int lw_r1cs_matvec(const lw_r1cs_t *r1cs, const void *z, size_t n_out, void *out_az_or_null, void *out_bz_or_null, void *out_cz_or_null) {
    return matvec_entry(r1cs, z, n_out, out_az_or_null, out_bz_or_null, out_cz_or_null, nullptr, false);
}
int lw_r1cs_matvec_device(const lw_r1cs_t *r1cs, const void *d_z, size_t n_out, void *d_out_az_or_null, void *d_out_bz_or_null,
                          void *d_out_cz_or_null, void *hip_stream) {
    return matvec_entry(r1cs, d_z, n_out, d_out_az_or_null, d_out_bz_or_null, d_out_cz_or_null, hip_stream, true);
}

static int bind_entry(const lw_r1cs_t *h, const void *e, const void *coeffs3, size_t n_out, void *out, void *hip_stream, bool device) {
    if (!h || !e || !coeffs3 || !out) return r1cs_null();
    if (n_out < h->n_cols || n_out > R1CS_MAX_OUT) { set_error("n_out = %zu: from the %u columns to 2^34", n_out, h->n_cols); return LW_ERR_BAD_ARG; }
    const size_t eb = (size_t)h->n_rows * 32, ob = n_out * 32;
    if (device && (!ml_aligned16(e) || !ml_aligned16(out))) return r1cs_misaligned();
    if (ml_overlap(out, ob, e, eb)) { set_error("the output overlaps e"); return LW_ERR_BAD_ARG; }
    Entry en(hip_stream);
    if (en.rc) return en.rc;
    Context &c = en.c;
    if (device) return r1cs_bind_locked(c, h, e, coeffs3, n_out, out, en.stream);
    hipStream_t s = en.use_lane_stream();
    if (!s) return en.rc;
    if (c.host_io_b.ensure(ob)) return LW_ERR_ALLOC;   // both buffers before any copy from caller memory
    int rc = ml_upload(c.host_io_a, e, eb, s);
    if (rc) return rc;
    rc = r1cs_bind_locked(c, h, c.host_io_a.p, coeffs3, n_out, c.host_io_b.p, s);
    return rc ? rc : ml_download(out, c.host_io_b.p, ob, s);
}
int lw_r1cs_bind_rows(const lw_r1cs_t *r1cs, const void *e, const void *coeffs3, size_t n_out, void *out) {
    return bind_entry(r1cs, e, coeffs3, n_out, out, nullptr, false);
}
int lw_r1cs_bind_rows_device(const lw_r1cs_t *r1cs, const void *d_e, const void *coeffs3, size_t n_out, void *d_out, void *hip_stream) {
    return bind_entry(r1cs, d_e, coeffs3, n_out, d_out, hip_stream, true);
}

static int check_entry(const lw_r1cs_t *h, const void *z, int64_t *out_row, void *hip_stream, bool device) {
    if (!h || !z || !out_row) return r1cs_null();
    if (device && !ml_aligned16(z)) return r1cs_misaligned();
    Entry en(hip_stream);
    if (en.rc) return en.rc;
    Context &c = en.c;
    if (device) return r1cs_check_locked(c, h, z, out_row, en.stream);
    hipStream_t s = en.use_lane_stream();
    if (!s) return en.rc;
    int rc = ml_upload(c.host_io_a, z, (size_t)h->n_cols * 32, s);
    return rc ? rc : r1cs_check_locked(c, h, c.host_io_a.p, out_row, s);
}
int lw_r1cs_first_unsatisfied(const lw_r1cs_t *r1cs, const void *z, int64_t *out_row) {
    return check_entry(r1cs, z, out_row, nullptr, false);
}
int lw_r1cs_first_unsatisfied_device(const lw_r1cs_t *r1cs, const void *d_z, int64_t *out_row, void *hip_stream) {
    return check_entry(r1cs, d_z, out_row, hip_stream, true);
}

}  // extern "C"
