// The Merkle tree of an algebraic hash and the host side of its entry points, written once for poseidon.hip, rpo.hip,
// pedersen.hip and monolith.hip: three kernels, the schedule that launches them, the argument checks and the entry bodies
// (flat batches and commit_columns).  A hash is a compile-time policy H, a struct of constants and static
// __device__ __forceinline__ functions over byte addresses, so every kernel holds a single inlined copy of H's permutation:
//   H::DIGEST_BYTES, H::ELEM_BYTES             a digest (a tree node), an input element
//   H::parent(x, y, out)                       out = the parent of the digests at x and at y
//   H::row(row, len, elem_stride, mode, out)   out = the digest of the `len` elements row[c * elem_stride], c = 0 .. len - 1;
//                                              `mode` is H's own (Poseidon's leaf rule), wave-uniform like len
//   H::ready(c)                                host: whatever parent and row read beyond their arguments (a table of the
//                                              library, table_once below) is on the device; LW_OK at once if there is none.
//                                              tree_pair_device and tree_rows_device call it before they launch, inside the
//                                              call's one Entry, so a table and the kernels that read it share one hold of
//                                              the lane and of SharedState::rw: no lw_hip_init can move the library between them
#pragma once
#include <string.h>
#include <initializer_list>
#include "internal.h"

namespace lw {

// out[i] = parent of x[i * stride], y[i * stride], strides in digests: a flat 2-to-1 hash (two arrays, stride 1) or a wide
// tree level (x = the children, y = x + one digest, stride 2)
template <class H> __global__ __launch_bounds__(256) void tree_pair_kernel(const char *x, const char *y, uint64_t stride, uint64_t n, char *out) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    H::parent(x + i * stride * H::DIGEST_BYTES, y + i * stride * H::DIGEST_BYTES, out + i * H::DIGEST_BYTES);
}

// Digest i of n: H::row over the elements base[src * row_stride + c * elem_stride], with src = i, or the bit reversal of i
// over `bitrev_bits` bits (bitrev_bits >= 0).  The flat hashes over row-major rows and the leaves over strided columns.
template <class H>
__global__ __launch_bounds__(256) void tree_rows_kernel(const char *base, uint64_t n, uint32_t len, uint64_t row_stride, uint64_t elem_stride,
                                                        int bitrev_bits, int mode, char *out) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint64_t src = bitrev_bits < 0 ? i : (bitrev_bits ? (uint64_t)(__brevll(i) >> (64 - bitrev_bits)) : 0);
    H::row(base + src * row_stride * H::ELEM_BYTES, len, elem_stride, mode, out + i * H::DIGEST_BYTES);
}

// The top of a tree in one launch, as merkle_top_kernel: every level from the one starting at node level_begin (at most 512
// nodes, level_end its last) down to the root, one parent per work-item, a barrier between levels.
template <class H> __global__ __launch_bounds__(256) void tree_top_kernel(char *nodes, uint64_t level_begin, uint64_t level_end) {
    constexpr uint64_t D = H::DIGEST_BYTES;
    while (level_begin != level_end) {
        const uint64_t new_begin = level_begin / 2, count = level_begin - new_begin;
        const uint64_t k = threadIdx.x;
        if (k < count) {
            const char *ch = nodes + (level_begin + 2 * k) * D;
            H::parent(ch, ch + D, nodes + (new_begin + k) * D);
        }
        // workgroup scope is enough, the children of the next level were written by this workgroup, and it is what the
        // kernel can afford: an agent-scope release writes back the whole L2 of the XCD (measured in merkle.hip)
        __threadfence_block();
        __syncthreads();
        level_end = level_begin - 1;
        level_begin = new_begin;
    }
}

static uint32_t blocks_for(uint64_t n) { return (uint32_t)((n + 255) / 256); }
// one checked launch of `blocks` workgroups of 256; `name` is the kernel's line in the profile
template <class... P, class... A>
static int launch_1d(Context &c, const char *name, void (*kernel)(P...), uint32_t blocks, hipStream_t s, A... args) {
    hipEvent_t pe = c.prof_begin(s);
    hipLaunchKernelGGL(kernel, dim3(blocks), dim3(256), 0, s, (P)args...);
    c.prof_end(name, pe, s);
    LW_HIP_CHECK(hipGetLastError(), LW_ERR_LAUNCH);
    return LW_OK;
}

struct TreeNames { const char *rows, *pair, *top; };   // the profile lines of a hash's three kernels

// A table of the library (a __device__ or __constant__ variable), filled from `host` before the first kernel that reads it
// is enqueued.  `ready` lives with the shared state (one table per device, whichever lane asks first) and is cleared when
// the device changes.
template <class T> static int table_once(Context &c, bool &ready, const T &symbol, const void *host, size_t bytes) {
    if (ready) return LW_OK;
    ExclusiveScope excl(c);
    if (ready) return LW_OK;
    LW_HIP_CHECK(hipMemcpyToSymbol(HIP_SYMBOL(symbol), host, bytes), LW_ERR_LAUNCH);
    LW_HIP_CHECK(hipStreamSynchronize(nullptr), LW_ERR_LAUNCH);   // the lanes' streams do not wait for the null stream
    ready = true;
    return LW_OK;
}

template <class H>
static int tree_pair_device(Context &c, const char *name, const void *d_x, const void *d_y, uint64_t stride, uint64_t n, void *d_out, hipStream_t s) {
    const int rc = H::ready(c);
    return rc ? rc : launch_1d(c, name, tree_pair_kernel<H>, blocks_for(n), s, d_x, d_y, stride, n, d_out);
}
template <class H>
static int tree_rows_device(Context &c, const char *name, const void *d_base, uint64_t n, uint32_t len, uint64_t row_stride, uint64_t elem_stride,
                            int bitrev_bits, int mode, void *d_out, hipStream_t s) {
    const int rc = H::ready(c);
    return rc ? rc : launch_1d(c, name, tree_rows_kernel<H>, blocks_for(n), s, d_base, n, len, row_stride, elem_stride, bitrev_bits, mode, d_out);
}

// d_nodes: (2 * 2^log2n - 1) digests, root first (crypto/src/merkle_tree/utils.rs:43-71: the level of 2^m nodes starts at
// node 2^m - 1).  Leaf j is H::row over element j (its bit reversal with bit_reverse) of every column.
// Schedule, from the arithmetic (thresholds NOT MEASURED against alternatives; profiles/poseidon.txt and profiles/rpo.txt
// time this one).  A work-item's permutation is long next to the ~10 us of a dependent launch, for either of two reasons:
//   Poseidon  a dependent chain of 214 products, latency bound: ~75 us for a wave at the measured fe_mul rate (VERDICT:
//             189 G products/s over 1024 SIMDs), so a level of up to 65 536 parents takes about that long however it is
//             launched and a launch is a tenth of it.  Measured: 1 x 2^24 in 46.2 ms, 0.75 of the 214-product ceiling,
//             1 x 2^20 in 5.8 ms, 0.38 - its narrow levels come to ~0.2 ms each, so a lone wave's chain is slower still.
//   RPO       6384 (8512) gl_mul that a wave issues one after the other: with m chains side by side the wave is bound by
//             issue, not by latency, so a lone wave takes 6384 x 64 lanes / (the per-SIMD product rate) whatever else
//             runs - 255 us (340 us) at the measured 1637 G products/s over 1024 SIMDs, and a launch is a few
//             hundredths of it.  Measured: 8 x 2^20 in 16.9 ms (26.8 ms), 0.48 (0.41) of the product ceiling.
// Hence:
//   * no levels fused into the leaf kernel or into one another (the Keccak tree's fuse = 4 / FUSE_BELOW = 16): in a fused
//     launch level k + 1 runs on half the work-items of level k while the others hold their slots - a whole permutation
//     time spent to save a launch a tenth as long or less; every wide level is one launch of the pair kernel, stride 2;
//   * the top kernel takes over at 256 parents (TOP_LOG2 = 9: a level of 2^9 nodes), one parent per work-item of one
//     workgroup, its four waves on the four SIMDs of one CU: from there every level is one permutation time on one CU or
//     on many, and the barrier replaces 9 launches.  A larger top (1024 parents on the 16 waves of one workgroup) would
//     put 4 waves on each SIMD of one CU where a launch spreads them over 16 SIMDs: slower per level (four times, where
//     the waves are issue bound) than the launch it saves.
template <class H>
static int tree_commit_device(Context &c, const TreeNames &names, const void *d_cols, uint32_t n_cols, uint64_t col_stride, uint32_t log2n,
                              int bit_reverse, int mode, void *d_nodes, hipStream_t s) {
    constexpr uint32_t TOP_LOG2 = 9;
    constexpr uint64_t D = H::DIGEST_BYTES;
    const uint64_t n = 1ull << log2n;
    char *nodes = (char *)d_nodes;
    int rc = tree_rows_device<H>(c, names.rows, d_cols, n, n_cols, 1, col_stride, bit_reverse ? (int)log2n : -1, mode, nodes + (n - 1) * D, s);
    if (rc) return rc;
    uint32_t m = log2n;   // the level whose parents are built next holds 2^m nodes
    for (; m > TOP_LOG2; m--) {
        const char *children = nodes + ((1ull << m) - 1) * D;
        rc = tree_pair_device<H>(c, names.pair, children, children + D, 2, 1ull << (m - 1), nodes + ((1ull << (m - 1)) - 1) * D, s);
        if (rc) return rc;
    }
    if (m == 0) return LW_OK;
    const uint64_t level_begin = (1ull << m) - 1;
    return launch_1d(c, names.top, tree_top_kernel<H>, 1, s, nodes, level_begin, 2 * level_begin);
}

// ---- argument helpers of the entry points
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
// `count` items (`noun`: what they are, at most `limit`); every pointer in bufs must be there (and 16-byte aligned for the
// _device forms) once there is work
static int flat_check(uint64_t count, uint64_t limit, const char *noun, std::initializer_list<const void *> bufs, bool device) {
    if (count > limit) { set_error("%llu %s inputs", (unsigned long long)count, noun); return LW_ERR_ALLOC; }
    if (count == 0) return LW_OK;
    for (const void *p : bufs) {
        if (!p) { set_error("null buffer"); return LW_ERR_BAD_ARG; }
        if (device && !aligned16(p)) { set_error("device buffers must be 16-byte aligned"); return LW_ERR_BAD_ARG; }
    }
    return LW_OK;
}
// n_rows rows of row_len `unit`s ("elements", "words"), row_stride >= row_len apart; rows may be null when row_len = 0:
// no row data is read
static int rows_check(size_t n_rows, size_t row_len, size_t row_stride, uint64_t limit, const char *noun, const char *unit, const void *rows,
                      const void *out, bool device) {
    if (row_stride < row_len) { set_error("row stride %zu below the row length %zu", row_stride, row_len); return LW_ERR_BAD_ARG; }
    if (row_len > ((size_t)1 << 31) || (row_stride && n_rows > (limit << 4) / row_stride)) {
        set_error("%zu rows of %zu %s", n_rows, row_stride, unit);
        return LW_ERR_ALLOC;
    }
    return row_len ? flat_check(n_rows, limit, noun, {rows, out}, device) : flat_check(n_rows, limit, noun, {out}, device);
}
// both commitment forms, after the hash's own lines; nodes_or_root: d_nodes (device form) or out_root (host form);
// col_stride in elements, 0 = dense
static int tree_commit_check(const void *columns, const void *nodes_or_root, uint32_t n_cols, uint64_t col_stride, uint32_t log2n,
                             uint32_t max_log2n, bool device) {
    if (!columns || !nodes_or_root || n_cols == 0) { set_error("null buffer or no columns"); return LW_ERR_BAD_ARG; }
    if (device && (!aligned16(columns) || !aligned16(nodes_or_root))) { set_error("device buffers must be 16-byte aligned"); return LW_ERR_BAD_ARG; }
    if (log2n > max_log2n) { set_error("2^%u leaves", log2n); return LW_ERR_ALLOC; }
    if (col_stride && col_stride < (1ull << log2n)) {
        set_error("column stride %llu below the column length", (unsigned long long)col_stride);
        return LW_ERR_BAD_ARG;
    }
    return LW_OK;
}

// ---- the body of a flat entry point, after its checks: `in` are the one or two inputs (pointer, bytes), `out` the output.
// Device form: run(c, the caller's inputs, out, the caller's stream), enqueued only.  Host form, complete on return: the
// inputs staged back to back in host_io_a on the lane's stream (an empty one is not copied), run, the output downloaded
// from host_io_b, or with in_place from host_io_a, where run overwrote input 0.
struct FlatIn { const void *p; size_t bytes; };
template <class Run>
static int flat_entry(void *hip_stream, bool device, std::initializer_list<FlatIn> in, void *out, size_t out_bytes, bool in_place, Run run) {
    Entry en(hip_stream);
    if (en.rc) return en.rc;
    const void *d_in[2];
    int k = 0;
    if (device) {
        for (const FlatIn &i : in) d_in[k++] = i.p;
        return run(en.c, d_in, out, en.stream);
    }
    hipStream_t s = en.use_lane_stream();
    if (!s) return en.rc;
    Context &c = en.c;
    size_t in_bytes = 0;
    for (const FlatIn &i : in) in_bytes += i.bytes;
    if (c.host_io_a.ensure(in_bytes ? in_bytes : 16) || (!in_place && c.host_io_b.ensure(out_bytes))) return LW_ERR_ALLOC;
    char *at = (char *)c.host_io_a.p;
    int rc = LW_OK;
    for (const FlatIn &i : in) {
        if (!rc && i.bytes) rc = upload(at, i.p, i.bytes, s);
        d_in[k++] = at;
        at += i.bytes;
    }
    void *d_out = in_place ? c.host_io_a.p : c.host_io_b.p;
    if (!rc) rc = run(c, d_in, d_out, s);
    return rc ? rc : download(out, d_out, out_bytes, s);
}
// the two flat hashes of H as entry bodies: out[i] = parent(x[i], y[i]); out[i] = H::row of row i, the rows row_stride
// apart (the host form's are dense: row_stride = row_len)
template <class H>
static int tree_pair_entry(const char *name, const void *x, const void *y, size_t n, void *out, void *hip_stream, bool device) {
    const size_t bytes = n * H::DIGEST_BYTES;
    return flat_entry(hip_stream, device, {{x, bytes}, {y, bytes}}, out, bytes, false, [&](Context &c, const void *const *d_in, void *d_out, hipStream_t s) {
        return tree_pair_device<H>(c, name, d_in[0], d_in[1], 1, n, d_out, s);
    });
}
template <class H>
static int tree_rows_entry(const char *name, const void *rows, size_t n_rows, size_t row_len, size_t row_stride, int mode, void *out,
                           void *hip_stream, bool device) {
    return flat_entry(hip_stream, device, {{rows, n_rows * row_len * H::ELEM_BYTES}}, out, n_rows * H::DIGEST_BYTES, false,
                      [&](Context &c, const void *const *d_in, void *d_out, hipStream_t s) {
                          return tree_rows_device<H>(c, name, d_in[0], n_rows, (uint32_t)row_len, row_stride, 1, -1, mode, d_out, s);
                      });
}

// ---- the bodies of commit_columns, after the argument checks
// device form: col_stride in elements, 0 = dense; the root goes to out_root (the stream is waited for) unless it is null
template <class H>
static int tree_commit_columns_device(const TreeNames &names, const void *d_columns, uint32_t n_cols, uint64_t col_stride, uint32_t log2n,
                                      int bit_reverse, int mode, void *d_nodes, void *out_root, void *hip_stream) {
    Entry en(hip_stream);
    if (en.rc) return en.rc;
    if (col_stride == 0) col_stride = 1ull << log2n;
    const int rc = tree_commit_device<H>(en.c, names, d_columns, n_cols, col_stride, log2n, bit_reverse, mode, d_nodes, en.stream);
    if (rc) return rc;
    return out_root ? download(out_root, d_nodes, H::DIGEST_BYTES, en.stream) : LW_OK;
}
// host form: dense columns in, the root and (unless null) all nodes out
template <class H>
static int tree_commit_columns_host(const TreeNames &names, const void *columns, uint32_t n_cols, uint32_t log2n, int bit_reverse, int mode,
                                    void *out_root, void *out_nodes_or_null) {
    const size_t n = (size_t)1 << log2n, in_bytes = (size_t)n_cols * n * H::ELEM_BYTES, node_bytes = (2 * n - 1) * H::DIGEST_BYTES;
    Entry en(nullptr);
    if (en.rc) return en.rc;
    Context &c = en.c;
    hipStream_t s = en.use_lane_stream();
    if (!s) return en.rc;
    if (c.host_io_a.ensure(in_bytes) || c.host_io_b.ensure(node_bytes)) return LW_ERR_ALLOC;
    int rc = upload(c.host_io_a.p, columns, in_bytes, s);
    if (!rc) rc = tree_commit_device<H>(c, names, c.host_io_a.p, n_cols, n, log2n, bit_reverse, mode, c.host_io_b.p, s);
    if (rc) return rc;
    if (!out_nodes_or_null) return download(out_root, c.host_io_b.p, H::DIGEST_BYTES, s);
    rc = download(out_nodes_or_null, c.host_io_b.p, node_bytes, s);
    if (!rc) memcpy(out_root, out_nodes_or_null, H::DIGEST_BYTES);
    return rc;
}

}  // namespace lw
