// Rescue Prime Optimized over Goldilocks on the device: batched permutations and hashes, and the Merkle tree built from
// the reference's `hash` (crypto/src/hash/rescue_prime/rescue_prime_optimized.rs:192-230).  The permutation itself and
// its bounds are in rpo.cuh.
//
// Here: rpo_permute_kernel (n states of m words, permutation), the hash policy RpoHash<LEVEL> (hash, and the parent
// hash(left || right)), the one place where the run-time level picks the template argument, the argument checks and the
// exported entry points.  hash_tree.cuh has the rest, once for this hash and for Poseidon: the pair, rows and top kernels
// around RpoHash, the tree schedule and the commit_columns bodies.
// A permutation is 6384 (8512) Goldilocks products against at most a few hundred bytes of traffic, so the accesses are
// left as they fall (rows of a row-major matrix, a bit-reversed gather of the columns): nothing is transposed or copied.
#include "hash_tree.cuh"
#include "rpo.cuh"

namespace lw {

template <int LEVEL> __global__ __launch_bounds__(256) void rpo_permute_kernel(const uint64_t *in, uint64_t *out, uint64_t n) {
    constexpr int M = RpoParams<LEVEL>::M;
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint64_t s[M];
#pragma unroll
    for (int j = 0; j < M; j++) s[j] = gl_from_word(in[i * M + j]);
    rpo_permute<LEVEL>(s);
#pragma unroll
    for (int j = 0; j < M; j++) out[i * M + j] = s[j];
}

template <int LV> struct RpoHash {   // the policy of hash_tree.cuh: an element is a word, a digest DIGEST words
    typedef RpoParams<LV> R;
    static constexpr int LEVEL = LV;
    static constexpr uint64_t DIGEST_BYTES = R::DIGEST * 8, ELEM_BYTES = 8;
    static int ready(Context &) { return LW_OK; }   // the constants come with the code object
    // hash(left || right): 2 * DIGEST = RATE words, so one full block, word 0 of the state 0, one permutation at both
    // levels.  The digests are canonical (the kernels wrote them).
    static __device__ __forceinline__ void parent(const char *x, const char *y, char *out) {
        static_assert(2 * R::DIGEST == R::RATE, "a pair of digests is one block");
        uint64_t s[R::M];
#pragma unroll
        for (int j = 0; j < R::CAP; j++) s[j] = 0;
#pragma unroll
        for (int j = 0; j < R::DIGEST; j++) s[R::CAP + j] = gl_from_word(((const uint64_t *)x)[j]);
#pragma unroll
        for (int j = 0; j < R::DIGEST; j++) s[R::CAP + R::DIGEST + j] = gl_from_word(((const uint64_t *)y)[j]);
        rpo_permute<LV>(s);
#pragma unroll
        for (int j = 0; j < R::DIGEST; j++) ((uint64_t *)out)[j] = s[R::CAP + j];
    }
    // hash (rescue_prime_optimized.rs:205-230) of the `len` words row[c * elem_stride].  Word 0 of the state is 1 iff len is
    // no multiple of the rate; every block OVERWRITES the rate part; a partial last block is the words, a 1, zeros; len = 0
    // runs no permutation and the digest is zeros.  len and the block count are wave-uniform.
    // mode is a group size g (0: none): word c of the row is element (c mod g) (len / g) + c / g, so that `len / g` columns of
    // each of g vectors hash element after element (the Fp2 FRI layer of goldilocks_ext.hip: g = 2 planes).  g divides len.
    static __device__ __forceinline__ void row(const char *row, uint32_t len, uint64_t elem_stride, int mode, char *out) {
        uint64_t s[R::M];
#pragma unroll
        for (int j = 0; j < R::M; j++) s[j] = 0;
        if (len % R::RATE) s[0] = 1;
        const uint32_t blocks = (len + R::RATE - 1) / R::RATE;
        const uint32_t g = (uint32_t)mode, per = g ? len / g : 0;
        for (uint32_t b = 0; b < blocks; b++) {
#pragma unroll
            for (int h = 0; h < R::RATE; h++) {
                const uint32_t c = b * R::RATE + h;   // wave-uniform
                uint32_t e = c;
                if (g && c < len) e = (c % g) * per + c / g;
                s[R::CAP + h] = c < len ? gl_from_word(((const uint64_t *)row)[(uint64_t)e * elem_stride]) : (c == len ? 1 : 0);
            }
            rpo_permute<LV>(s);
        }
#pragma unroll
        for (int j = 0; j < R::DIGEST; j++) ((uint64_t *)out)[j] = s[R::CAP + j];
    }
};
static constexpr TreeNames RPO_NAMES = {"rpo_sponge_kernel", "rpo_pair_kernel", "rpo_top_kernel"};

// The run-time level becomes the template argument here and nowhere else: f(RpoHash<0>()) or f(RpoHash<1>()).
template <class F> static int rpo_with_level(int level, F f) { return level == LW_RPO_128 ? f(RpoHash<0>()) : f(RpoHash<1>()); }

// ---- argument checks: one per entry-point family, run before any device work
static constexpr uint64_t RPO_MAX_N = (uint64_t)1 << 36;   // the grid's block index stays below 2^31
int rpo_level_check(int level) {
    if (level != LW_RPO_128 && level != LW_RPO_160) { set_error("bad RPO level %d", level); return LW_ERR_BAD_ARG; }
    return LW_OK;
}

int rpo_commit_locked(Context &c, int level, const uint64_t *d_columns, uint32_t n_cols, uint64_t col_stride, uint32_t log2n, int bit_reverse,
                      int group, uint64_t *d_nodes, hipStream_t stream) {
    return rpo_with_level(level, [&](auto h) {
        return tree_commit_device<decltype(h)>(c, RPO_NAMES, d_columns, n_cols, col_stride, log2n, bit_reverse, group, d_nodes, stream);
    });
}

}  // namespace lw

using namespace lw;

extern "C" {

static int permute_entry(int level, const void *states, size_t n, void *out, void *hip_stream, bool device) {
    int rc = rpo_level_check(level);
    if (!rc) rc = flat_check(n, RPO_MAX_N, "RPO", {states, out}, device);
    if (rc || n == 0) return rc;
    return rpo_with_level(level, [&](auto h) {
        const size_t bytes = n * decltype(h)::R::M * 8;
        return flat_entry(hip_stream, device, {{states, bytes}}, out, bytes, true, [&](Context &c, const void *const *d_in, void *d_out, hipStream_t s) {
            return launch_1d(c, "rpo_permute_kernel", rpo_permute_kernel<decltype(h)::LEVEL>, blocks_for(n), s, d_in[0], d_out, (uint64_t)n);
        });
    });
}
int lw_rpo_permute(lw_rpo_level_t level, const uint64_t *states, size_t n, uint64_t *out) { return permute_entry(level, states, n, out, nullptr, false); }
int lw_rpo_permute_device(lw_rpo_level_t level, const uint64_t *d_states, size_t n, uint64_t *d_out, void *hip_stream) {
    return permute_entry(level, d_states, n, d_out, hip_stream, true);
}

static int hash_entry(int level, const void *rows, size_t n_rows, size_t row_len, size_t row_stride, void *out, void *hip_stream,
                      bool device) {
    if (row_stride == 0) row_stride = row_len;
    int rc = rpo_level_check(level);
    if (!rc) rc = rows_check(n_rows, row_len, row_stride, RPO_MAX_N, "RPO", "words", rows, out, device);
    if (rc || n_rows == 0) return rc;
    return rpo_with_level(level, [&](auto h) {
        return tree_rows_entry<decltype(h)>(RPO_NAMES.rows, rows, n_rows, row_len, row_stride, 0, out, hip_stream, device);
    });
}
int lw_rpo_hash(lw_rpo_level_t level, const uint64_t *rows, size_t n_rows, size_t row_len, uint64_t *out) {
    return hash_entry(level, rows, n_rows, row_len, 0, out, nullptr, false);
}
int lw_rpo_hash_device(lw_rpo_level_t level, const uint64_t *d_rows, size_t n_rows, size_t row_len, size_t row_stride, uint64_t *d_out,
                       void *hip_stream) {
    return hash_entry(level, d_rows, n_rows, row_len, row_stride, d_out, hip_stream, true);
}

// checks of both commitment forms; nodes_or_root: d_nodes (device form) or out_root (host form)
static int commit_check(int level, const void *columns, const void *nodes_or_root, uint32_t n_cols, uint64_t col_stride, uint32_t log2n,
                        bool device) {
    const int rc = rpo_level_check(level);
    return rc ? rc : tree_commit_check(columns, nodes_or_root, n_cols, col_stride, log2n, 30, device);
}
int lw_rpo_commit_columns_device(lw_rpo_level_t level, const uint64_t *d_columns, uint32_t n_cols, uint64_t col_stride, uint32_t log2n,
                                 int bit_reverse, uint64_t *d_nodes, uint64_t *out_root, void *hip_stream) {
    const int rc = commit_check(level, d_columns, d_nodes, n_cols, col_stride, log2n, true);
    if (rc) return rc;
    return rpo_with_level(level, [&](auto h) {
        return tree_commit_columns_device<decltype(h)>(RPO_NAMES, d_columns, n_cols, col_stride, log2n, bit_reverse, 0, d_nodes, out_root, hip_stream);
    });
}
int lw_rpo_commit_columns(lw_rpo_level_t level, const uint64_t *columns, uint32_t n_cols, uint32_t log2n, int bit_reverse, uint64_t *out_root,
                          uint64_t *out_nodes_or_null) {
    const int rc = commit_check(level, columns, out_root, n_cols, 0, log2n, false);
    if (rc) return rc;
    return rpo_with_level(level, [&](auto h) {
        return tree_commit_columns_host<decltype(h)>(RPO_NAMES, columns, n_cols, log2n, bit_reverse, 0, out_root, out_nodes_or_null);
    });
}

}  // extern "C"
