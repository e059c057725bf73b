// Monolith over Mersenne31 on the device: batched permutations for the five widths of the reference
// (crypto/src/hash/monolith/, MonolithMersenne31<WIDTH, NUM_FULL_ROUNDS>) and, for width 16, the two hashing modes Plonky3
// builds from the permutation for this field and the Merkle tree made of them.  The layers and their bounds are in
// monolith.cuh.
//
// Here: the constants (generated on the host from their SHAKE128 rule, one __constant__ table of the library for every
// (width, rounds), uploaded once per device), monolith_permute_kernel and the test seam monolith_layer_kernel (one state
// per work-item), the hash policy MonolithHash<R> for hash_tree.cuh, the places where the run-time width and round count
// pick the template argument, the argument checks and the exported entry points.
//
// Why a table of the library and a policy per round count: the policy functions of hash_tree.cuh are static, so what a
// parent hash needs beyond its two children has to be reachable without an argument.  The round count is the template
// argument, the constants sit at fixed addresses, and every read of them is a scalar load from the constant address space.
// A permutation is 256 (R + 2) multiply-adds against 64 bytes in and out, so the accesses are left as they fall.
#include <string.h>
#include <mutex>
#include <type_traits>
#include "hash_tree.cuh"
#include "monolith.cuh"

namespace lw {

// ---- the table: widths 8 + 4 wi, wi = 0 .. 4; rounds 1 .. 15
// rc:  the R rows of (W, R) start at word RC_BASE[wi] + W R (R - 1) / 2   (120 W words per width, 9600 in all)
// mds: the W x W matrix of (W, R) starts at word MDS_BASE[wi] + W W (R - 1)   (15 W W words per width, 21600 in all; for
//      W = 16 it is the circulant written out, which only lw_monolith_constants reads)
constexpr uint32_t MONOLITH_RC_WORDS = 9600, MONOLITH_MDS_WORDS = 21600;
constexpr uint32_t MONOLITH_RC_BASE[5] = {0, 960, 2400, 4320, 6720};
constexpr uint32_t MONOLITH_MDS_BASE[5] = {0, 960, 3120, 6960, 12960};
struct MonolithTable {
    uint32_t rc[MONOLITH_RC_WORDS];
    uint32_t mds[MONOLITH_MDS_WORDS];
};
__constant__ MonolithTable MONOLITH_TABLE;

template <int W> __host__ __device__ __forceinline__ const uint32_t *monolith_rc_of(const MonolithTable &t, uint32_t rounds) {
    return t.rc + MONOLITH_RC_BASE[(W - 8) / 4] + W * (rounds * (rounds - 1) / 2);
}
template <int W> __host__ __device__ __forceinline__ const uint32_t *monolith_mds_of(const MonolithTable &t, uint32_t rounds) {
    return t.mds + MONOLITH_MDS_BASE[(W - 8) / 4] + W * W * (rounds - 1);
}

// ---- SHAKE128 on the host, over the Keccak-f[1600] of stark_query.hip; the seeds here are shorter than one block
struct Shake128Words {   // the stream as little-endian u32 words (168 bytes = 42 words per block)
    uint64_t st[25] = {0};
    int at = 0;
    Shake128Words(const uint8_t *seed, size_t len) {
        uint8_t block[168] = {0};
        memcpy(block, seed, len);
        block[len] = 0x1F;
        block[167] |= 0x80;
        for (int i = 0; i < 21; i++)
            for (int b = 7; b >= 0; b--) st[i] = (st[i] << 8) | block[8 * i + b];
        keccak_f1600_host(st);
    }
    uint32_t next() {
        if (at == 42) {
            keccak_f1600_host(st);
            at = 0;
        }
        const uint32_t w = (uint32_t)(st[at / 2] >> (32 * (at % 2)));
        at++;
        return w;
    }
};

// instantiate_round_constants (mod.rs:47-55) and the matrix of concrete (:105-118, 152-174; utils.rs:12-55) of one instance
static void monolith_generate(uint32_t W, uint32_t R, uint32_t *rc, uint32_t *mds) {
    uint8_t seed[21] = {'M', 'o', 'n', 'o', 'l', 'i', 't', 'h', (uint8_t)W, (uint8_t)(R + 1), 0xFF, 0xFF, 0xFF, 0x7F, 8, 8, 8, 7};
    Shake128Words rounds_stream(seed, 18);
    for (uint32_t k = 0; k < R * W; k++) {
        uint32_t v = rounds_stream.next();
        while (v >= M31_P) v = rounds_stream.next();
        rc[k] = v;
    }
    if (W == 16) {
        for (int i = 0; i < 16; i++)
            for (int j = 0; j < 16; j++) mds[i * 16 + j] = MONOLITH_CIRC16[(j - i) & 15];
        return;
    }
    memcpy(seed + 14, "\x10\x0fMDS", 5);
    Shake128Words mds_stream(seed, 19);
    const uint32_t x_mask = (1u << 22) - 1, y_mask = M31_P >> 2;
    uint32_t y[24];
    for (uint32_t i = 0; i < W; i++) {
        bool again = true;
        while (again) {   // redraw while the x part collides with an earlier one
            y[i] = mds_stream.next() & y_mask;
            again = false;
            for (uint32_t k = 0; k < i; k++) again |= (y[k] & x_mask) == (y[i] & x_mask);
        }
    }
    for (uint32_t i = 0; i < W; i++)
        for (uint32_t j = 0; j < W; j++) mds[i * W + j] = m31_canon(m31_inv(m31_add(y[i] & x_mask, y[j])));
}

static const MonolithTable &monolith_host_table() {   // every instance, generated once per process (75 short SHAKE128 streams)
    static MonolithTable table;
    static std::once_flag once;
    std::call_once(once, [] {
        for (uint32_t wi = 0; wi < 5; wi++)
            for (uint32_t R = 1; R <= (uint32_t)MONOLITH_MAX_ROUNDS; R++) {
                const uint32_t W = 8 + 4 * wi;
                monolith_generate(W, R, table.rc + MONOLITH_RC_BASE[wi] + W * (R * (R - 1) / 2), table.mds + MONOLITH_MDS_BASE[wi] + W * W * (R - 1));
            }
    });
    return table;
}
static int monolith_ready(Context &c) {   // before the first kernel that reads MONOLITH_TABLE is enqueued
    return table_once(c, shared_state().monolith_table_ready, MONOLITH_TABLE, &monolith_host_table(), sizeof(MonolithTable));
}

// ---- kernels: one state per work-item; a state is W words, 16-byte aligned (W is a multiple of 4)
template <int W> __device__ __forceinline__ void monolith_load(const uint32_t *p, uint32_t (&s)[W]) {
#pragma unroll
    for (int q = 0; q < W / 4; q++) {
        const uint4 v = ((const uint4 *)p)[q];
        s[4 * q] = m31_from_word(v.x);
        s[4 * q + 1] = m31_from_word(v.y);
        s[4 * q + 2] = m31_from_word(v.z);
        s[4 * q + 3] = m31_from_word(v.w);
    }
}
template <int W> __device__ __forceinline__ void monolith_store(uint32_t *p, const uint32_t (&s)[W]) {   // canonical words out
#pragma unroll
    for (int q = 0; q < W / 4; q++)
        ((uint4 *)p)[q] = make_uint4(m31_canon(s[4 * q]), m31_canon(s[4 * q + 1]), m31_canon(s[4 * q + 2]), m31_canon(s[4 * q + 3]));
}

template <int W> __global__ __launch_bounds__(256) void monolith_permute_kernel(const uint32_t *in, uint32_t *out, uint64_t n, uint32_t rounds) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint32_t s[W];
    monolith_load<W>(in + i * W, s);
    monolith_permute<W>(s, rounds, monolith_rc_of<W>(MONOLITH_TABLE, rounds), monolith_mds_of<W>(MONOLITH_TABLE, rounds));
    monolith_store<W>(out + i * W, s);
}

// Test seam: one layer per state, the very function the permutation inlines, so that chosen words can stand in front of Bars
// and Concrete
template <int W> __global__ __launch_bounds__(256) void monolith_layer_kernel(const uint32_t *in, uint32_t *out, uint64_t n, uint32_t rounds, int layer) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint32_t s[W];
    monolith_load<W>(in + i * W, s);
    if (layer == LW_MONOLITH_CONCRETE) monolith_concrete<W>(s, monolith_mds_of<W>(MONOLITH_TABLE, rounds));
    else if (layer == LW_MONOLITH_BARS) monolith_bars<W>(s);
    else monolith_bricks<W>(s);
    monolith_store<W>(out + i * W, s);
}

// The policy of hash_tree.cuh over the width-16 permutation with R rounds: an element is a word, a digest 8 words.
template <int R> struct MonolithHash {
    static constexpr uint64_t DIGEST_BYTES = 32, ELEM_BYTES = 4;
    static int ready(Context &c) { return monolith_ready(c); }
    static __device__ __forceinline__ void permute(uint32_t (&s)[16]) { monolith_permute<16>(s, R, monolith_rc_of<16>(MONOLITH_TABLE, R), nullptr); }
    // compress: permute(left || right)[0..8]
    static __device__ __forceinline__ void parent(const char *x, const char *y, char *out) {
        uint32_t l[8], r[8], s[16];
        monolith_load<8>((const uint32_t *)x, l);
        monolith_load<8>((const uint32_t *)y, r);
#pragma unroll
        for (int j = 0; j < 8; j++) s[j] = l[j], s[8 + j] = r[j];
        permute(s);
#pragma unroll
        for (int j = 0; j < 8; j++) l[j] = s[j];
        monolith_store<8>((uint32_t *)out, l);
    }
    // hash of the `len` words row[c * elem_stride]: the state starts as zeros, every chunk of up to 8 words OVERWRITES the
    // front of the state and the rest stays, one permutation per chunk, no padding; len = 0 runs none and the digest is
    // zeros.  len and the chunk count are wave-uniform.  No mode.
    static __device__ __forceinline__ void row(const char *row, uint32_t len, uint64_t elem_stride, int, char *out) {
        uint32_t s[16], d[8];
#pragma unroll
        for (int j = 0; j < 16; j++) s[j] = 0;
        for (uint32_t at = 0; at < len; at += 8) {
#pragma unroll
            for (int h = 0; h < 8; h++)
                if (at + h < len) s[h] = m31_from_word(((const uint32_t *)row)[(uint64_t)(at + h) * elem_stride]);   // wave-uniform
            permute(s);
        }
#pragma unroll
        for (int j = 0; j < 8; j++) d[j] = s[j];
        monolith_store<8>((uint32_t *)out, d);
    }
};
static constexpr TreeNames MONOLITH_NAMES = {"monolith_sponge_kernel", "monolith_pair_kernel", "monolith_top_kernel"};

// The run-time round count and width become template arguments here and nowhere else: f(MonolithHash<R>()),
// f(std::integral_constant<int, W>()).  Both were checked by the caller.
template <class F> static int monolith_with_rounds(uint32_t rounds, F f) {
    switch (rounds) {
#define LW_MONOLITH_ROUNDS(R) case R: return f(MonolithHash<R>());
        LW_MONOLITH_ROUNDS(1) LW_MONOLITH_ROUNDS(2) LW_MONOLITH_ROUNDS(3) LW_MONOLITH_ROUNDS(4) LW_MONOLITH_ROUNDS(5)
        LW_MONOLITH_ROUNDS(6) LW_MONOLITH_ROUNDS(7) LW_MONOLITH_ROUNDS(8) LW_MONOLITH_ROUNDS(9) LW_MONOLITH_ROUNDS(10)
        LW_MONOLITH_ROUNDS(11) LW_MONOLITH_ROUNDS(12) LW_MONOLITH_ROUNDS(13) LW_MONOLITH_ROUNDS(14) LW_MONOLITH_ROUNDS(15)
#undef LW_MONOLITH_ROUNDS
    }
    return LW_ERR_BAD_ARG;
}
template <class F> static int monolith_with_width(uint32_t width, F f) {
    switch (width) {
        case 8: return f(std::integral_constant<int, 8>());
        case 12: return f(std::integral_constant<int, 12>());
        case 16: return f(std::integral_constant<int, 16>());
        case 20: return f(std::integral_constant<int, 20>());
        case 24: return f(std::integral_constant<int, 24>());
    }
    return LW_ERR_BAD_ARG;
}

static int monolith_permute_device(Context &c, uint32_t width, uint32_t rounds, const void *d_in, void *d_out, uint64_t n, hipStream_t s) {
    const int rc = monolith_ready(c);
    if (rc) return rc;
    return monolith_with_width(width, [&](auto w) {
        return launch_1d(c, "monolith_permute_kernel", monolith_permute_kernel<decltype(w)::value>, blocks_for(n), s, d_in, d_out, n, rounds);
    });
}

// ---- argument checks: one per entry-point family, run before any device work
static constexpr uint64_t MONOLITH_MAX_N = (uint64_t)1 << 36;   // the grid's block index stays below 2^31
static int rounds_check(uint32_t rounds) {
    if (rounds < 1 || rounds > (uint32_t)MONOLITH_MAX_ROUNDS) { set_error("Monolith rounds %u: 1 .. %d", rounds, MONOLITH_MAX_ROUNDS); return LW_ERR_BAD_ARG; }
    return LW_OK;
}
static int instance_check(uint32_t width, uint32_t rounds) {
    if (width < 8 || width > 24 || width % 4) { set_error("Monolith width %u: 8, 12, 16, 20 or 24", width); return LW_ERR_BAD_ARG; }
    return rounds_check(rounds);
}

}  // namespace lw

using namespace lw;

extern "C" {

int lw_monolith_constants(uint32_t width, uint32_t rounds, uint32_t *out_round_constants, uint32_t *out_mds) {
    const int rc = instance_check(width, rounds);
    if (rc) return rc;
    if (!out_round_constants || !out_mds) { set_error("null buffer"); return LW_ERR_BAD_ARG; }
    const MonolithTable &t = monolith_host_table();
    const uint32_t wi = (width - 8) / 4;
    memcpy(out_round_constants, t.rc + MONOLITH_RC_BASE[wi] + width * (rounds * (rounds - 1) / 2), (size_t)rounds * width * 4);
    memcpy(out_mds, t.mds + MONOLITH_MDS_BASE[wi] + width * width * (rounds - 1), (size_t)width * width * 4);
    return LW_OK;
}

static int permute_entry(uint32_t width, uint32_t rounds, const void *states, size_t n, void *out, void *hip_stream, bool device) {
    int rc = instance_check(width, rounds);
    if (!rc) rc = flat_check(n, MONOLITH_MAX_N, "Monolith", {states, out}, device);
    if (rc || n == 0) return rc;
    const size_t bytes = n * width * 4;
    return flat_entry(hip_stream, device, {{states, bytes}}, out, bytes, true, [&](Context &c, const void *const *d_in, void *d_out, hipStream_t s) {
        return monolith_permute_device(c, width, rounds, d_in[0], d_out, n, s);
    });
}
int lw_monolith_permute(uint32_t width, uint32_t rounds, const uint32_t *states, size_t n, uint32_t *out) {
    return permute_entry(width, rounds, states, n, out, nullptr, false);
}
int lw_monolith_permute_device(uint32_t width, uint32_t rounds, const uint32_t *d_states, size_t n, uint32_t *d_out, void *hip_stream) {
    return permute_entry(width, rounds, d_states, n, d_out, hip_stream, true);
}

static int hash_entry(uint32_t rounds, const void *rows, size_t n_rows, size_t row_len, size_t row_stride, void *out, void *hip_stream,
                      bool device) {
    if (row_stride == 0) row_stride = row_len;
    int rc = rounds_check(rounds);
    if (!rc) rc = rows_check(n_rows, row_len, row_stride, MONOLITH_MAX_N, "Monolith", "words", rows, out, device);
    if (rc || n_rows == 0) return rc;
    return monolith_with_rounds(rounds, [&](auto h) {
        return tree_rows_entry<decltype(h)>(MONOLITH_NAMES.rows, rows, n_rows, row_len, row_stride, 0, out, hip_stream, device);
    });
}
int lw_monolith_hash(uint32_t rounds, const uint32_t *rows, size_t n_rows, size_t row_len, uint32_t *out) {
    return hash_entry(rounds, rows, n_rows, row_len, 0, out, nullptr, false);
}
int lw_monolith_hash_device(uint32_t rounds, const uint32_t *d_rows, size_t n_rows, size_t row_len, size_t row_stride, uint32_t *d_out,
                            void *hip_stream) {
    return hash_entry(rounds, d_rows, n_rows, row_len, row_stride, d_out, hip_stream, true);
}

static int compress_entry(uint32_t rounds, const void *left, const void *right, size_t n, void *out, void *hip_stream, bool device) {
    int rc = rounds_check(rounds);
    if (!rc) rc = flat_check(n, MONOLITH_MAX_N, "Monolith", {left, right, out}, device);
    if (rc || n == 0) return rc;
    return monolith_with_rounds(rounds, [&](auto h) {
        return tree_pair_entry<decltype(h)>(MONOLITH_NAMES.pair, left, right, n, out, hip_stream, device);
    });
}
int lw_monolith_compress(uint32_t rounds, const uint32_t *left, const uint32_t *right, size_t n, uint32_t *out) {
    return compress_entry(rounds, left, right, n, out, nullptr, false);
}
int lw_monolith_compress_device(uint32_t rounds, const uint32_t *d_left, const uint32_t *d_right, size_t n, uint32_t *d_out, void *hip_stream) {
    return compress_entry(rounds, d_left, d_right, n, d_out, hip_stream, true);
}

int lw_monolith_layer_device(uint32_t width, uint32_t rounds, lw_monolith_layer_t layer, const uint32_t *d_states, size_t n, uint32_t *d_out,
                             void *hip_stream) {
    int rc = instance_check(width, rounds);
    if (rc) return rc;
    if (layer != LW_MONOLITH_CONCRETE && layer != LW_MONOLITH_BARS && layer != LW_MONOLITH_BRICKS) {
        set_error("bad Monolith layer %d", (int)layer);
        return LW_ERR_BAD_ARG;
    }
    rc = flat_check(n, MONOLITH_MAX_N, "Monolith", {d_states, d_out}, true);
    if (rc || n == 0) return rc;
    Entry en(hip_stream);
    if (en.rc) return en.rc;
    rc = monolith_ready(en.c);
    if (rc) return rc;
    return monolith_with_width(width, [&](auto w) {
        return launch_1d(en.c, "monolith_layer_kernel", monolith_layer_kernel<decltype(w)::value>, blocks_for(n), en.stream, d_states, d_out,
                         (uint64_t)n, rounds, (int)layer);
    });
}

// checks of both commitment forms; nodes_or_root: d_nodes (device form) or out_root (host form)
static int commit_check(uint32_t rounds, const void *columns, const void *nodes_or_root, uint32_t n_cols, uint64_t col_stride, uint32_t log2n,
                        bool device) {
    const int rc = rounds_check(rounds);
    return rc ? rc : tree_commit_check(columns, nodes_or_root, n_cols, col_stride, log2n, 30, device);
}
int lw_monolith_commit_columns_device(uint32_t rounds, const uint32_t *d_columns, uint32_t n_cols, uint64_t col_stride, uint32_t log2n,
                                      int bit_reverse, uint32_t *d_nodes, uint32_t *out_root, void *hip_stream) {
    const int rc = commit_check(rounds, d_columns, d_nodes, n_cols, col_stride, log2n, true);
    if (rc) return rc;
    return monolith_with_rounds(rounds, [&](auto h) {
        return tree_commit_columns_device<decltype(h)>(MONOLITH_NAMES, d_columns, n_cols, col_stride, log2n, bit_reverse, 0, d_nodes, out_root, hip_stream);
    });
}
int lw_monolith_commit_columns(uint32_t rounds, const uint32_t *columns, uint32_t n_cols, uint32_t log2n, int bit_reverse, uint32_t *out_root,
                               uint32_t *out_nodes_or_null) {
    const int rc = commit_check(rounds, columns, out_root, n_cols, 0, log2n, false);
    if (rc) return rc;
    return monolith_with_rounds(rounds, [&](auto h) {
        return tree_commit_columns_host<decltype(h)>(MONOLITH_NAMES, columns, n_cols, log2n, bit_reverse, 0, out_root, out_nodes_or_null);
    });
}

}  // extern "C"
