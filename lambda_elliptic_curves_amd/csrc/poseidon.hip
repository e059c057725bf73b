// Starknet Poseidon on the device: batched permutations and hashes, and the Poseidon Merkle trees of the reference
// (crypto/src/merkle_tree/backends/field_element.rs:53-76 TreePoseidon, field_element_vector.rs:61-85 BatchPoseidonTree,
// both with P = PoseidonCairoStark252).  The permutation itself and its bounds are in poseidon.cuh.
//
// Four kernels, one work-item per permutation chain, each with a single inlined copy of the permutation:
//   poseidon_permute_kernel   n states of 3 elements                                   hades_permutation
//   poseidon_pair_kernel      out[i] = hash(x[i], y[i]), x and y strided               hash; a wide tree level (stride 2)
//   poseidon_sponge_kernel    one digest per row, elements gathered by two strides     hash_single, hash_many, tree leaves
//   poseidon_top_kernel       the last <= 256 parents down to the root, one workgroup  the top of a tree
// A node costs 214 Montgomery products against a few hundred bytes of traffic, so the accesses are left as they fall
// (rows of a row-major matrix, a bit-reversed gather of the columns): nothing is transposed, tiled or copied first.
#include <string.h>
#include <initializer_list>
#include "internal.h"
#include "poseidon.cuh"

namespace lw {

__device__ __forceinline__ PFe poseidon_small(uint32_t v) {   // 0, 1 or 2 in Montgomery form
    PFe r = PFe::zero();
    if (v >= 1) r = PFe::one();
    if (v == 2) r = fe_add<Stark252>(r, r);
    return r;
}

__global__ __launch_bounds__(256) void poseidon_permute_kernel(const char *in, char *out, uint64_t n) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    PFe s[3];
#pragma unroll
    for (int j = 0; j < 3; j++) s[j] = fe_load<Stark252>(in + (3 * i + j) * 32);
    poseidon_permute(s);
#pragma unroll
    for (int j = 0; j < 3; j++) fe_store<Stark252>(out + (3 * i + j) * 32, s[j]);
}

// out[i] = word 0 of permute(x[i * stride], y[i * stride], 2), strides in elements (mod.rs:59-64)
__global__ __launch_bounds__(256) void poseidon_pair_kernel(const char *x, const char *y, uint64_t stride, uint64_t n, char *out) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    PFe s[3] = {fe_load<Stark252>(x + i * stride * 32), fe_load<Stark252>(y + i * stride * 32), poseidon_small(2)};
    poseidon_permute(s);
    fe_store<Stark252>(out + i * 32, s[0]);
}

// Digest i of n: the sponge over the `len` elements base[src * row_stride + c * elem_stride], c = 0 .. len - 1, with
// src = i, or the bit reversal of i over `bitrev_bits` bits (bitrev_bits >= 0).
//   single = 0, hash_many (mod.rs:73-96): the elements, a 1, zeros up to a multiple of 2; two per permutation are added
//               to words 0 and 1 of a state that starts at zero; len / 2 + 1 permutations (len = 0: the padding alone)
//   single = 1, hash_single (mod.rs:66-71): len = 1, one permutation of (x, 0, 1)
__global__ __launch_bounds__(256) void poseidon_sponge_kernel(const char *base, uint64_t n, uint32_t len, uint64_t row_stride,
                                                              uint64_t elem_stride, int bitrev_bits, int single, char *out) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint64_t src = bitrev_bits < 0 ? i : (bitrev_bits ? (uint64_t)(__brevll(i) >> (64 - bitrev_bits)) : 0);
    const char *row = base + src * row_stride * 32;
    PFe s[3] = {PFe::zero(), PFe::zero(), poseidon_small(single ? 1 : 0)};
    const uint32_t blocks = single ? 1 : len / 2 + 1;
    for (uint32_t b = 0; b < blocks; b++) {
#pragma unroll
        for (int h = 0; h < 2; h++) {
            const uint32_t c = 2 * b + h;   // wave-uniform
            PFe e;
            if (c < len) e = fe_load<Stark252>(row + (uint64_t)c * elem_stride * 32);
            else e = poseidon_small(c == len && !single ? 1 : 0);
            s[h] = fe_add<Stark252>(s[h], e);   // both canonical
        }
        poseidon_permute(s);
    }
    fe_store<Stark252>(out + i * 32, s[0]);
}

// The top of a tree in one launch, as merkle_top_kernel: every level from the one starting at node level_begin (at most 512
// nodes, level_end its last) down to the root, one parent per work-item, a barrier between levels.
__global__ __launch_bounds__(256) void poseidon_top_kernel(char *nodes, uint64_t level_begin, uint64_t level_end) {
    while (level_begin != level_end) {
        const uint64_t new_begin = level_begin / 2, count = level_begin - new_begin;
        const uint64_t k = threadIdx.x;
        if (k < count) {
            const char *ch = nodes + (level_begin + 2 * k) * 32;
            PFe s[3] = {fe_load<Stark252>(ch), fe_load<Stark252>(ch + 32), poseidon_small(2)};
            poseidon_permute(s);
            fe_store<Stark252>(nodes + (new_begin + k) * 32, s[0]);
        }
        __threadfence_block();   // workgroup scope is enough: the children of the next level were written by this workgroup
        __syncthreads();
        level_end = level_begin - 1;
        level_begin = new_begin;
    }
}

static dim3 grid_for(uint64_t n) { return dim3((uint32_t)((n + 255) / 256)); }

static int poseidon_permute_device(Context &c, const void *d_in, void *d_out, uint64_t n, hipStream_t s) {
    hipEvent_t pe = c.prof_begin(s);
    hipLaunchKernelGGL(poseidon_permute_kernel, grid_for(n), dim3(256), 0, s, (const char *)d_in, (char *)d_out, n);
    c.prof_end("poseidon_permute_kernel", pe, s);
    LW_HIP_CHECK(hipGetLastError(), LW_ERR_LAUNCH);
    return LW_OK;
}
static int poseidon_pair_device(Context &c, const void *d_x, const void *d_y, uint64_t stride, uint64_t n, void *d_out, hipStream_t s) {
    hipEvent_t pe = c.prof_begin(s);
    hipLaunchKernelGGL(poseidon_pair_kernel, grid_for(n), dim3(256), 0, s, (const char *)d_x, (const char *)d_y, stride, n, (char *)d_out);
    c.prof_end("poseidon_pair_kernel", pe, s);
    LW_HIP_CHECK(hipGetLastError(), LW_ERR_LAUNCH);
    return LW_OK;
}
static int poseidon_sponge_device(Context &c, const void *d_base, uint64_t n, uint32_t len, uint64_t row_stride, uint64_t elem_stride,
                                  int bitrev_bits, int single, void *d_out, hipStream_t s) {
    hipEvent_t pe = c.prof_begin(s);
    hipLaunchKernelGGL(poseidon_sponge_kernel, grid_for(n), dim3(256), 0, s, (const char *)d_base, n, len, row_stride, elem_stride,
                       bitrev_bits, single, (char *)d_out);
    c.prof_end("poseidon_sponge_kernel", pe, s);
    LW_HIP_CHECK(hipGetLastError(), LW_ERR_LAUNCH);
    return LW_OK;
}

// d_nodes: (2 * 2^log2n - 1) elements, root first (crypto/src/merkle_tree/utils.rs:43-71: the level of 2^m nodes starts at
// node 2^m - 1).
// Schedule, from the arithmetic (thresholds NOT MEASURED against alternatives; profiles/poseidon.txt times this one: 1 x 2^24 in
// 46.3 ms, 0.75 of the 214-product ceiling, 1 x 2^20 in 5.8 ms, 0.37 — its narrow levels come to ~0.2 ms each, so a lone wave's
// chain is slower than the estimate that follows): a permutation is a dependent chain of 214
// products, ~75 us for a wave at the measured fe_mul rate (VERDICT: 189 G products/s over 1024 SIMDs), so a level of up
// to 65 536 parents takes about that long however it is launched and the ~10 us of a dependent launch is a tenth of it.
//   * no levels fused into the leaf kernel or into one another (the Keccak tree's fuse = 4 / FUSE_BELOW = 16): in a fused
//     launch level k + 1 runs on half the work-items of level k while the others hold their slots — a whole permutation
//     latency spent to save a launch a tenth as long; every wide level is one launch of the pair kernel, stride 2;
//   * the top kernel takes over at 256 parents (TOP_LOG2 = 9: a level of 2^9 nodes), one parent per work-item of one
//     workgroup: from there every level is one permutation latency on one CU or on many, and the barrier replaces 9
//     launches.  A larger top (1024 parents on the 16 waves of one workgroup) would put 4 waves on each SIMD of one CU
//     where a launch spreads them over 16 SIMDs: slower per level than the launch it saves.
static int poseidon_commit_device(Context &c, const void *d_cols, uint32_t n_cols, uint64_t col_stride, uint32_t log2n, int bit_reverse,
                                  int leaf_mode, void *d_nodes, hipStream_t s) {
    constexpr uint32_t TOP_LOG2 = 9;
    const uint64_t n = 1ull << log2n;
    char *nodes = (char *)d_nodes;
    int rc = poseidon_sponge_device(c, d_cols, n, n_cols, 1, col_stride, bit_reverse ? (int)log2n : -1,
                                    leaf_mode == LW_POSEIDON_LEAF_SINGLE, nodes + (n - 1) * 32, s);
    if (rc) return rc;
    uint32_t m = log2n;   // the level whose parents are built next holds 2^m nodes
    for (; m > TOP_LOG2; m--) {
        const char *children = nodes + ((1ull << m) - 1) * 32;
        rc = poseidon_pair_device(c, children, children + 32, 2, 1ull << (m - 1), nodes + ((1ull << (m - 1)) - 1) * 32, s);
        if (rc) return rc;
    }
    if (m > 0) {
        const uint64_t level_begin = (1ull << m) - 1;
        hipEvent_t pe = c.prof_begin(s);
        hipLaunchKernelGGL(poseidon_top_kernel, dim3(1), dim3(256), 0, s, nodes, level_begin, 2 * level_begin);
        c.prof_end("poseidon_top_kernel", pe, s);
        LW_HIP_CHECK(hipGetLastError(), LW_ERR_LAUNCH);
    }
    return LW_OK;
}

// ---- argument checks: one per entry-point family, run before any device work
static constexpr uint64_t POSEIDON_MAX_N = (uint64_t)1 << 36;   // the grid's block index stays below 2^31
static bool aligned16(const void *p) { return ((uintptr_t)p & 15) == 0; }
static int upload(void *dst, const void *src, size_t bytes, hipStream_t s) {
    LW_HIP_CHECK(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, s), LW_ERR_LAUNCH);
    return LW_OK;
}
static int download(void *dst, const void *src, size_t bytes, hipStream_t s) {   // complete on return
    LW_HIP_CHECK(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, s), LW_ERR_LAUNCH);
    LW_HIP_CHECK(hipStreamSynchronize(s), LW_ERR_LAUNCH);
    return LW_OK;
}
// `count` items; every pointer in bufs must be there (and 16-byte aligned for the _device forms) once there is work
static int flat_check(uint64_t count, std::initializer_list<const void *> bufs, bool device) {
    if (count > POSEIDON_MAX_N) { set_error("%llu Poseidon inputs", (unsigned long long)count); return LW_ERR_ALLOC; }
    if (count == 0) return LW_OK;
    for (const void *p : bufs) {
        if (!p) { set_error("null buffer"); return LW_ERR_BAD_ARG; }
        if (device && !aligned16(p)) { set_error("device buffers must be 16-byte aligned"); return LW_ERR_BAD_ARG; }
    }
    return LW_OK;
}

}  // namespace lw

using namespace lw;

extern "C" {

static int permute_entry(const void *states, size_t n, void *out, void *hip_stream, bool device) {
    const int rc = flat_check(n, {states, out}, device);
    if (rc || n == 0) return rc;
    Entry en(hip_stream);
    if (en.rc) return en.rc;
    if (device) return poseidon_permute_device(en.c, states, out, n, en.stream);
    hipStream_t s = en.use_lane_stream();
    if (!s) return en.rc;
    Context &c = en.c;
    if (c.host_io_a.ensure(n * 96)) return LW_ERR_ALLOC;
    int r = upload(c.host_io_a.p, states, n * 96, s);
    if (!r) r = poseidon_permute_device(c, c.host_io_a.p, c.host_io_a.p, n, s);
    return r ? r : download(out, c.host_io_a.p, n * 96, s);
}
int lw_poseidon_permute(const void *states, size_t n, void *out) { return permute_entry(states, n, out, nullptr, false); }
int lw_poseidon_permute_device(const void *d_states, size_t n, void *d_out, void *hip_stream) {
    return permute_entry(d_states, n, d_out, hip_stream, true);
}

static int hash_entry(const void *x, const void *y, size_t n, void *out, void *hip_stream, bool device) {
    const int rc = flat_check(n, {x, y, out}, device);
    if (rc || n == 0) return rc;
    Entry en(hip_stream);
    if (en.rc) return en.rc;
    if (device) return poseidon_pair_device(en.c, x, y, 1, n, out, en.stream);
    hipStream_t s = en.use_lane_stream();
    if (!s) return en.rc;
    Context &c = en.c;
    if (c.host_io_a.ensure(n * 64) || c.host_io_b.ensure(n * 32)) return LW_ERR_ALLOC;
    char *dx = (char *)c.host_io_a.p, *dy = dx + n * 32;
    int r = upload(dx, x, n * 32, s);
    if (!r) r = upload(dy, y, n * 32, s);
    if (!r) r = poseidon_pair_device(c, dx, dy, 1, n, c.host_io_b.p, s);
    return r ? r : download(out, c.host_io_b.p, n * 32, s);
}
int lw_poseidon_hash(const void *x, const void *y, size_t n, void *out) { return hash_entry(x, y, n, out, nullptr, false); }
int lw_poseidon_hash_device(const void *d_x, const void *d_y, size_t n, void *d_out, void *hip_stream) {
    return hash_entry(d_x, d_y, n, d_out, hip_stream, true);
}

// hash_single (single = true, row_len = 1) and hash_many
static int rows_entry(const void *rows, size_t n_rows, size_t row_len, bool single, void *out, void *hip_stream, bool device) {
    if (row_len > ((size_t)1 << 31) || (row_len && n_rows > (POSEIDON_MAX_N << 4) / row_len)) {
        set_error("%zu rows of %zu elements", n_rows, row_len);
        return LW_ERR_ALLOC;
    }
    int rc = row_len ? flat_check(n_rows, {rows, out}, device) : flat_check(n_rows, {out}, device);   // no row data: rows is not read
    if (rc || n_rows == 0) return rc;
    Entry en(hip_stream);
    if (en.rc) return en.rc;
    if (device) return poseidon_sponge_device(en.c, rows, n_rows, (uint32_t)row_len, row_len, 1, -1, single, out, en.stream);
    hipStream_t s = en.use_lane_stream();
    if (!s) return en.rc;
    Context &c = en.c;
    const size_t in_bytes = n_rows * row_len * 32;
    if (c.host_io_a.ensure(in_bytes ? in_bytes : 32) || c.host_io_b.ensure(n_rows * 32)) return LW_ERR_ALLOC;
    int r = in_bytes ? upload(c.host_io_a.p, rows, in_bytes, s) : LW_OK;
    if (!r) r = poseidon_sponge_device(c, c.host_io_a.p, n_rows, (uint32_t)row_len, row_len, 1, -1, single, c.host_io_b.p, s);
    return r ? r : download(out, c.host_io_b.p, n_rows * 32, s);
}
int lw_poseidon_hash_single(const void *x, size_t n, void *out) { return rows_entry(x, n, 1, true, out, nullptr, false); }
int lw_poseidon_hash_single_device(const void *d_x, size_t n, void *d_out, void *hip_stream) {
    return rows_entry(d_x, n, 1, true, d_out, hip_stream, true);
}
int lw_poseidon_hash_many(const void *rows, size_t n_rows, size_t row_len, void *out) {
    return rows_entry(rows, n_rows, row_len, false, out, nullptr, false);
}
int lw_poseidon_hash_many_device(const void *d_rows, size_t n_rows, size_t row_len, void *d_out, void *hip_stream) {
    return rows_entry(d_rows, n_rows, row_len, false, d_out, hip_stream, true);
}

// checks of both commitment forms; nodes_or_root: d_nodes (device form) or out_root (host form)
static int commit_check(const void *columns, const void *nodes_or_root, uint32_t n_cols, uint32_t log2n, int leaf_mode, bool device) {
    if (!columns || !nodes_or_root || n_cols == 0) { set_error("null buffer or no columns"); return LW_ERR_BAD_ARG; }
    if (leaf_mode != LW_POSEIDON_LEAF_SINGLE && leaf_mode != LW_POSEIDON_LEAF_MANY) { set_error("bad leaf mode %d", leaf_mode); return LW_ERR_BAD_ARG; }
    if (leaf_mode == LW_POSEIDON_LEAF_SINGLE && n_cols != 1) {
        set_error("LW_POSEIDON_LEAF_SINGLE (TreePoseidon) commits one column, not %u", n_cols);
        return LW_ERR_BAD_ARG;
    }
    if (device && (!aligned16(columns) || !aligned16(nodes_or_root))) { set_error("device buffers must be 16-byte aligned"); return LW_ERR_BAD_ARG; }
    if (log2n > 31) { set_error("2^%u leaves", log2n); return LW_ERR_ALLOC; }
    return LW_OK;
}
int lw_poseidon_commit_columns_device(const void *d_columns, uint32_t n_cols, uint64_t col_stride_elems, uint32_t log2n, int bit_reverse,
                                      int leaf_mode, void *d_nodes, uint8_t *out_root, void *hip_stream) {
    int rc = commit_check(d_columns, d_nodes, n_cols, log2n, leaf_mode, true);
    if (rc) return rc;
    Entry en(hip_stream);
    if (en.rc) return en.rc;
    if (col_stride_elems == 0) col_stride_elems = 1ull << log2n;
    rc = poseidon_commit_device(en.c, d_columns, n_cols, col_stride_elems, log2n, bit_reverse, leaf_mode, d_nodes, en.stream);
    if (rc) return rc;
    return out_root ? download(out_root, d_nodes, 32, en.stream) : LW_OK;
}
int lw_poseidon_commit_columns(const void *columns, uint32_t n_cols, uint32_t log2n, int bit_reverse, int leaf_mode, uint8_t *out_root,
                               uint8_t *out_nodes_or_null) {
    int rc = commit_check(columns, out_root, n_cols, log2n, leaf_mode, false);
    if (rc) return rc;
    const size_t n = (size_t)1 << log2n;
    Entry en(nullptr);
    if (en.rc) return en.rc;
    Context &c = en.c;
    hipStream_t s = en.use_lane_stream();
    if (!s) return en.rc;
    if (c.host_io_a.ensure((size_t)n_cols * n * 32) || c.host_io_b.ensure((2 * n - 1) * 32)) return LW_ERR_ALLOC;
    rc = upload(c.host_io_a.p, columns, (size_t)n_cols * n * 32, s);
    if (!rc) rc = poseidon_commit_device(c, c.host_io_a.p, n_cols, n, log2n, bit_reverse, leaf_mode, c.host_io_b.p, s);
    if (rc) return rc;
    if (out_nodes_or_null) {
        rc = download(out_nodes_or_null, c.host_io_b.p, (2 * n - 1) * 32, s);
        if (rc) return rc;
        memcpy(out_root, out_nodes_or_null, 32);
        return LW_OK;
    }
    return download(out_root, c.host_io_b.p, 32, s);
}

}  // extern "C"
