// The tail of the STARK prover's round 4 (provers/stark/src/prover.rs:596-617) on device-resident data:
//   grinding   grinding::generate_nonce (provers/stark/src/grinding.rs:40-54): the smallest nonce whose hash has
//              grinding_factor leading zero bits — one Keccak-f[1600] per candidate (stark_grind.cuh);
//   openings   fri::query_phase (fri/mod.rs:77-113), open_trace_polys and open_composition_poly (prover.rs:752-820):
//              MerkleTree::get_proof_by_pos (crypto/src/merkle_tree/merkle.rs:58-91, utils.rs:7-21) plus the committed
//              rows, gathered from the `nodes` arrays and columns that the commitment entry points left in HBM.
#include <string.h>
#include <vector>
#include "internal.h"
#include "stark_grind.cuh"

namespace lw {

// ---- grinding

// Keccak-f[1600] on the host: one permutation per call, for the inner hash (and for monolith.hip's SHAKE128)
void keccak_f1600_host(uint64_t (&a)[25]) {
    static const uint64_t RC[24] = {
        0x0000000000000001ULL, 0x0000000000008082ULL, 0x800000000000808aULL, 0x8000000080008000ULL, 0x000000000000808bULL,
        0x0000000080000001ULL, 0x8000000080008081ULL, 0x8000000000008009ULL, 0x000000000000008aULL, 0x0000000000000088ULL,
        0x0000000080008009ULL, 0x000000008000000aULL, 0x000000008000808bULL, 0x800000000000008bULL, 0x8000000000008089ULL,
        0x8000000000008003ULL, 0x8000000000008002ULL, 0x8000000000000080ULL, 0x000000000000800aULL, 0x800000008000000aULL,
        0x8000000080008081ULL, 0x8000000000008080ULL, 0x0000000080000001ULL, 0x8000000080008008ULL};
    auto rotl = [](uint64_t x, int n) { return (x << n) | (x >> (64 - n)); };
    for (int round = 0; round < 24; round++) {
        uint64_t bc[5];
        for (int i = 0; i < 5; i++) bc[i] = a[i] ^ a[i + 5] ^ a[i + 10] ^ a[i + 15] ^ a[i + 20];
        for (int i = 0; i < 5; i++) {
            const uint64_t t = bc[(i + 4) % 5] ^ rotl(bc[(i + 1) % 5], 1);
            for (int j = 0; j < 25; j += 5) a[j + i] ^= t;
        }
        uint64_t t = a[1];
        for (int i = 0; i < 24; i++) {
            const int j = GRIND_PIL[i];
            const uint64_t b = a[j];
            a[j] = rotl(t, GRIND_ROT[i]);
            t = b;
        }
        for (int j = 0; j < 25; j += 5) {
            for (int i = 0; i < 5; i++) bc[i] = a[j + i];
            for (int i = 0; i < 5; i++) a[j + i] = bc[i] ^ (~bc[(i + 1) % 5] & bc[(i + 2) % 5]);
        }
        a[0] ^= RC[round];
    }
}

// get_inner_hash (grinding.rs:70-79): Keccak256(PREFIX || seed || grinding_factor), 41 bytes, one block
static void grind_inner_hash(const uint8_t *seed32, uint32_t grinding_factor, uint8_t *out32) {
    uint8_t block[136] = {0x01, 0x23, 0x45, 0x67, 0x89, 0xab, 0xcd, 0xed};
    memcpy(block + 8, seed32, 32);
    block[40] = (uint8_t)grinding_factor;
    block[41] = 0x01;
    block[135] |= 0x80;
    uint64_t st[25] = {0};
    for (int i = 0; i < 17; i++)
        for (int b = 7; b >= 0; b--) st[i] = (st[i] << 8) | block[8 * i + b];
    keccak_f1600_host(st);
    for (int i = 0; i < 32; i++) out32[i] = (uint8_t)(st[i / 8] >> (8 * (i % 8)));
}

static int grind_check(const uint8_t *seed32, uint32_t grinding_factor, uint64_t first, uint64_t last, const uint64_t *out_nonce,
                       const int *out_found) {
    if (!seed32 || !out_nonce || !out_found) { set_error("null seed or output"); return LW_ERR_BAD_ARG; }
    if (grinding_factor < 1 || grinding_factor > 63) {
        set_error("grinding factor %u: 1 .. 63 (the limit is 1 << (64 - grinding_factor))", grinding_factor);
        return LW_ERR_BAD_ARG;
    }
    if (first > last) { set_error("empty nonce range"); return LW_ERR_BAD_ARG; }
    return LW_OK;
}

// [first, last] in ascending windows, one launch each; the first window with a hit holds the smallest valid nonce
static int grind_locked(Context &c, const uint8_t *seed32, uint32_t grinding_factor, uint64_t first, uint64_t last, uint64_t *out_nonce,
                        int *out_found, hipStream_t s) {
    // 2^64 - 1 is never a candidate: the reference iterates 0..u64::MAX (grinding.rs:45), and it is the value *best holds
    // while nothing is found.  last = 2^64 - 1 means 2^64 - 2; [2^64 - 1, 2^64 - 1] is empty.
    if (last == ~0ull) {
        if (first == ~0ull) {
            *out_found = 0;
            return LW_OK;
        }
        last = ~0ull - 1;
    }
    GrindArgs g;
    uint8_t inner[32];
    grind_inner_hash(seed32, grinding_factor, inner);
    grind_prepare(inner, g);
    g.shift = 64 - grinding_factor;
    if (c.small.ensure(256)) return LW_ERR_ALLOC;
    if (!c.pinned_words) LW_HIP_CHECK(hipHostMalloc((void **)&c.pinned_words, 256, hipHostMallocDefault), LW_ERR_ALLOC);
    unsigned long long *d_best = (unsigned long long *)c.small.p;
    volatile uint64_t *h_best = (volatile uint64_t *)(c.pinned_words + 40);   // words 0..31: MSM results, 32..39: a Merkle root
    LW_HIP_CHECK(hipMemsetAsync(d_best, 0xff, 8, s), LW_ERR_LAUNCH);
    const uint64_t window = grind_window(grinding_factor);
    *out_found = 0;
    for (uint64_t start = first;;) {
        const uint64_t end = last - start < window - 1 ? last : start + (window - 1);
        g.start = start;
        g.count = (uint32_t)(end - start + 1);
        const uint32_t blocks = (g.count + 255) / 256 < GRIND_MAX_BLOCKS ? (g.count + 255) / 256 : GRIND_MAX_BLOCKS;
        hipEvent_t pe = c.prof_begin(s);
        hipLaunchKernelGGL((grind_kernel<0>), dim3(blocks), dim3(256), 0, s, g, d_best);
        c.prof_end("grind_kernel", pe, s);
        LW_HIP_CHECK(hipGetLastError(), LW_ERR_LAUNCH);
        LW_HIP_CHECK(hipMemcpyAsync((void *)h_best, d_best, 8, hipMemcpyDeviceToHost, s), LW_ERR_LAUNCH);
        LW_HIP_CHECK(hipStreamSynchronize(s), LW_ERR_LAUNCH);
        if (*h_best != ~0ull) {
            *out_nonce = *h_best;
            *out_found = 1;
            return LW_OK;
        }
        if (end == last) return LW_OK;
        start = end + 1;
    }
}

// ---- openings

struct OpenTree {   // one tree of the call as the kernel reads it
    const uint64_t *cols;    // nullptr: paths only
    const uint64_t *nodes;
    uint64_t col_stride;     // elements
    uint32_t n_cols, log2_rows, rows_per_leaf, bit_reverse, log2_leaves;
    uint32_t values_per_query;   // rows_per_leaf * n_cols, 0 without columns
    uint64_t value_begin, path_begin;   // first 32-byte item of the tree in the values / in the paths
    uint64_t item_begin;     // first work-item of the tree: its values, then its paths
};

// One work-item per 32-byte item: an element of a committed row, or a node of an authentication path.
// out: [values of all trees | paths of all trees], each tree-major, then query.
__global__ __launch_bounds__(256) void open_trees_kernel(const OpenTree *trees, uint32_t n_trees, const uint64_t *positions, uint32_t q,
                                                         uint64_t n_items, uint64_t n_values, uint4 *out) {
    const uint64_t item = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (item >= n_items) return;
    uint32_t t = 0;
    while (t + 1 < n_trees && trees[t + 1].item_begin <= item) t++;
    const OpenTree tr = trees[t];
    uint64_t k = item - tr.item_begin;
    const uint64_t n_val = (uint64_t)q * tr.values_per_query;
    if (k < n_val) {   // element (row r of the leaf, column col) of query s
        const uint32_t s = (uint32_t)(k / tr.values_per_query), e = (uint32_t)(k % tr.values_per_query);
        const uint32_t r = e / tr.n_cols, col = e % tr.n_cols;
        const uint64_t j = positions[(uint64_t)t * q + s] * tr.rows_per_leaf + r;   // committed row
        const uint64_t row = tr.bit_reverse && tr.log2_rows ? (uint64_t)(__brevll(j) >> (64 - tr.log2_rows)) : j;
        const uint4 *src = (const uint4 *)(tr.cols + ((uint64_t)col * tr.col_stride + row) * 4);
        out[2 * (tr.value_begin + k)] = src[0];
        out[2 * (tr.value_begin + k) + 1] = src[1];
        return;
    }
    k -= n_val;        // node lvl of the path of query s, bottom first (build_merkle_path, merkle.rs:73-90)
    const uint32_t s = (uint32_t)(k / tr.log2_leaves), lvl = (uint32_t)(k % tr.log2_leaves);
    uint64_t i = positions[(uint64_t)t * q + s] + ((1ull << tr.log2_leaves) - 1);
    for (uint32_t l = 0; l < lvl; l++) i = (i - 1) >> 1;   // parent_index
    i = (i & 1) ? i + 1 : i - 1;                           // sibling_index; i >= 1 here
    const uint4 *src = (const uint4 *)(tr.nodes + i * 4);
    out[2 * (n_values + tr.path_begin + k)] = src[0];
    out[2 * (n_values + tr.path_begin + k) + 1] = src[1];
}

static int open_check(const lw_stark_tree_t *trees, uint32_t n_trees, const uint64_t *positions, uint32_t q, const void *out_values,
                      const uint8_t *out_paths) {
    if (!trees || !positions) { set_error("null tree table or positions"); return LW_ERR_BAD_ARG; }
    for (uint32_t t = 0; t < n_trees; t++) {
        const lw_stark_tree_t &tr = trees[t];
        if (tr.field != LW_FIELD_STARK252 && tr.field != LW_FIELD_BLS12_381_FR) {
            set_error("tree %u: openings support the 256-bit fields", t);
            return LW_ERR_BAD_ARG;
        }
        if (!tr.d_nodes) { set_error("tree %u: null nodes", t); return LW_ERR_BAD_ARG; }
        if (tr.rows_per_leaf != 1 && tr.rows_per_leaf != 2) { set_error("tree %u: %u rows per leaf", t, tr.rows_per_leaf); return LW_ERR_BAD_ARG; }
        if (tr.log2_rows > 31) { set_error("tree %u: 2^%u rows", t, tr.log2_rows); return LW_ERR_BAD_ARG; }
        if (tr.log2_rows == 0 && tr.rows_per_leaf == 2) { set_error("tree %u: one row cannot fill a leaf of two", t); return LW_ERR_BAD_ARG; }
        const uint64_t leaves = (1ull << tr.log2_rows) / tr.rows_per_leaf;
        if (tr.d_columns) {
            if (tr.n_cols == 0 || tr.n_cols > (1u << 20)) { set_error("tree %u: %u columns", t, tr.n_cols); return LW_ERR_BAD_ARG; }
            if (tr.col_stride_elems && tr.col_stride_elems < (1ull << tr.log2_rows)) { set_error("tree %u: column stride below the column length", t); return LW_ERR_BAD_ARG; }
            if (!out_values) { set_error("null out_values"); return LW_ERR_BAD_ARG; }
            if (((uintptr_t)tr.d_columns & 15) != 0) { set_error("tree %u: columns not 16-byte aligned", t); return LW_ERR_BAD_ARG; }
        }
        if (((uintptr_t)tr.d_nodes & 15) != 0) { set_error("tree %u: nodes not 16-byte aligned", t); return LW_ERR_BAD_ARG; }
        if (leaves > 1 && !out_paths) { set_error("null out_paths"); return LW_ERR_BAD_ARG; }
        for (uint32_t s = 0; s < q; s++)
            if (positions[(uint64_t)t * q + s] >= leaves) {
                set_error("tree %u: position %llu of %llu leaves", t, (unsigned long long)positions[(uint64_t)t * q + s], (unsigned long long)leaves);
                return LW_ERR_BAD_ARG;
            }
    }
    return LW_OK;
}

static int open_locked(Context &c, const lw_stark_tree_t *trees, uint32_t n_trees, const uint64_t *positions, uint32_t q, void *out_values,
                       uint8_t *out_paths, hipStream_t s) {
    // upload: [tree table | positions]; download: [values | paths]; both through the lane's pinned staging
    const size_t tab_b = ((size_t)n_trees * sizeof(OpenTree) + 255) & ~(size_t)255, pos_b = (size_t)n_trees * q * 8;
    const size_t up_b = (tab_b + pos_b + 255) & ~(size_t)255;
    std::vector<OpenTree> tab(n_trees);
    uint64_t n_values = 0, n_paths = 0, n_items = 0;
    for (uint32_t t = 0; t < n_trees; t++) {
        const lw_stark_tree_t &tr = trees[t];
        OpenTree &o = tab[t];
        o.cols = (const uint64_t *)tr.d_columns;
        o.nodes = (const uint64_t *)tr.d_nodes;
        o.col_stride = tr.col_stride_elems ? tr.col_stride_elems : 1ull << tr.log2_rows;
        o.n_cols = tr.n_cols;
        o.log2_rows = tr.log2_rows;
        o.rows_per_leaf = tr.rows_per_leaf;
        o.bit_reverse = tr.bit_reverse ? 1 : 0;
        o.log2_leaves = tr.log2_rows - (tr.rows_per_leaf - 1);
        o.values_per_query = tr.d_columns ? tr.rows_per_leaf * tr.n_cols : 0;
        o.value_begin = n_values;
        o.path_begin = n_paths;
        o.item_begin = n_items;
        n_values += (uint64_t)q * o.values_per_query;
        n_paths += (uint64_t)q * o.log2_leaves;
        n_items = n_values + n_paths;
    }
    if (n_items == 0) return LW_OK;   // single-leaf trees without columns: every path is empty
    const size_t down_b = (size_t)n_items * 32;
    if (c.pipe_tmp.ensure(up_b + down_b)) return LW_ERR_ALLOC;
    int rc = deep_pin(c, up_b + down_b);
    if (rc) return rc;
    char *h = (char *)c.deep_pin, *d = (char *)c.pipe_tmp.p;
    memset(h, 0, up_b);
    memcpy(h, tab.data(), (size_t)n_trees * sizeof(OpenTree));
    memcpy(h + tab_b, positions, pos_b);
    LW_HIP_CHECK(hipMemcpyAsync(d, h, up_b, hipMemcpyHostToDevice, s), LW_ERR_LAUNCH);
    hipEvent_t pe = c.prof_begin(s);
    hipLaunchKernelGGL(open_trees_kernel, dim3((uint32_t)((n_items + 255) / 256)), dim3(256), 0, s, (const OpenTree *)d,
                       n_trees, (const uint64_t *)(d + tab_b), q, n_items, n_values, (uint4 *)(d + up_b));
    c.prof_end("open_trees_kernel", pe, s);
    LW_HIP_CHECK(hipGetLastError(), LW_ERR_LAUNCH);
    LW_HIP_CHECK(hipMemcpyAsync(h + up_b, d + up_b, down_b, hipMemcpyDeviceToHost, s), LW_ERR_LAUNCH);
    LW_HIP_CHECK(hipEventRecord(c.deep_pin_read, s), LW_ERR_LAUNCH);
    LW_HIP_CHECK(hipStreamSynchronize(s), LW_ERR_LAUNCH);
    if (n_values) memcpy(out_values, h + up_b, (size_t)n_values * 32);
    if (n_paths) memcpy(out_paths, h + up_b + (size_t)n_values * 32, (size_t)n_paths * 32);
    return LW_OK;
}

}  // namespace lw

using namespace lw;

extern "C" {

uint64_t lw_stark_grinding_window(uint32_t grinding_factor) { return grind_window(grinding_factor); }

int lw_stark_grinding_nonce_device(const uint8_t *seed32, uint32_t grinding_factor, uint64_t first, uint64_t last, uint64_t *out_nonce,
                                   int *out_found, void *hip_stream) {
    const int rc = grind_check(seed32, grinding_factor, first, last, out_nonce, out_found);
    if (rc) return rc;
    Entry en(hip_stream);
    if (en.rc) return en.rc;
    return grind_locked(en.c, seed32, grinding_factor, first, last, out_nonce, out_found, en.stream);
}

int lw_stark_grinding_nonce(const uint8_t *seed32, uint32_t grinding_factor, uint64_t first, uint64_t last, uint64_t *out_nonce,
                            int *out_found) {
    const int rc = grind_check(seed32, grinding_factor, first, last, out_nonce, out_found);
    if (rc) return rc;
    Entry en(nullptr);
    if (en.rc) return en.rc;
    hipStream_t io = en.use_lane_stream();
    if (!io) return en.rc;
    return grind_locked(en.c, seed32, grinding_factor, first, last, out_nonce, out_found, io);
}

int lw_stark_open_trees_device(const lw_stark_tree_t *trees, uint32_t n_trees, const uint64_t *positions, uint32_t q, void *out_values,
                               uint8_t *out_paths, void *hip_stream) {
    if (q == 0 || n_trees == 0) return LW_OK;
    const int rc = open_check(trees, n_trees, positions, q, out_values, out_paths);
    if (rc) return rc;
    Entry en(hip_stream);
    if (en.rc) return en.rc;
    return open_locked(en.c, trees, n_trees, positions, q, out_values, out_paths, en.stream);
}

}  // extern "C"
