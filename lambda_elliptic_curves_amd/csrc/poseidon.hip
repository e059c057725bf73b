// Starknet Poseidon on the device: batched permutations and hashes, and the Poseidon Merkle trees of the reference
// (crypto/src/merkle_tree/backends/field_element.rs:53-76 TreePoseidon, field_element_vector.rs:61-85 BatchPoseidonTree,
// both with P = PoseidonCairoStark252).  The permutation itself and its bounds are in poseidon.cuh.
//
// Here: poseidon_permute_kernel (n states of 3 elements, hades_permutation), the hash policy PoseidonHash (hash,
// hash_single, hash_many), the argument checks and the exported entry points.  hash_tree.cuh has the rest, once for this
// hash and for RPO: the pair, rows and top kernels around PoseidonHash, the tree schedule and the commit_columns bodies.
// A node costs 214 Montgomery products against a few hundred bytes of traffic, so the accesses are left as they fall
// (rows of a row-major matrix, a bit-reversed gather of the columns): nothing is transposed, tiled or copied first.
#include "hash_tree.cuh"
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

struct PoseidonHash {   // the policy of hash_tree.cuh: an element and a digest are one Stark252 element
    static constexpr uint64_t DIGEST_BYTES = 32, ELEM_BYTES = 32;
    static int ready(Context &) { return LW_OK; }   // the round keys come with the code object
    // word 0 of permute(x, y, 2) (mod.rs:59-64)
    static __device__ __forceinline__ void parent(const char *x, const char *y, char *out) {
        PFe s[3] = {fe_load<Stark252>(x), fe_load<Stark252>(y), poseidon_small(2)};
        poseidon_permute(s);
        fe_store<Stark252>(out, s[0]);
    }
    // the sponge over the `len` elements row[c * elem_stride]:
    //   single = 0, hash_many (mod.rs:73-96): the elements, a 1, zeros up to a multiple of 2; two per permutation are added
    //               to words 0 and 1 of a state that starts at zero; len / 2 + 1 permutations (len = 0: the padding alone)
    //   single = 1, hash_single (mod.rs:66-71): len = 1, one permutation of (x, 0, 1)
    static __device__ __forceinline__ void row(const char *row, uint32_t len, uint64_t elem_stride, int single, char *out) {
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
        fe_store<Stark252>(out, s[0]);
    }
};
static constexpr TreeNames POSEIDON_NAMES = {"poseidon_sponge_kernel", "poseidon_pair_kernel", "poseidon_top_kernel"};

// ---- argument checks: one per entry-point family, run before any device work
static constexpr uint64_t POSEIDON_MAX_N = (uint64_t)1 << 36;   // the grid's block index stays below 2^31

}  // namespace lw

using namespace lw;

extern "C" {

static int permute_entry(const void *states, size_t n, void *out, void *hip_stream, bool device) {
    const int rc = flat_check(n, POSEIDON_MAX_N, "Poseidon", {states, out}, device);
    if (rc || n == 0) return rc;
    return flat_entry(hip_stream, device, {{states, n * 96}}, out, n * 96, true, [&](Context &c, const void *const *d_in, void *d_out, hipStream_t s) {
        return launch_1d(c, "poseidon_permute_kernel", poseidon_permute_kernel, blocks_for(n), s, d_in[0], d_out, (uint64_t)n);
    });
}
int lw_poseidon_permute(const void *states, size_t n, void *out) { return permute_entry(states, n, out, nullptr, false); }
int lw_poseidon_permute_device(const void *d_states, size_t n, void *d_out, void *hip_stream) {
    return permute_entry(d_states, n, d_out, hip_stream, true);
}

static int hash_entry(const void *x, const void *y, size_t n, void *out, void *hip_stream, bool device) {
    const int rc = flat_check(n, POSEIDON_MAX_N, "Poseidon", {x, y, out}, device);
    if (rc || n == 0) return rc;
    return tree_pair_entry<PoseidonHash>(POSEIDON_NAMES.pair, x, y, n, out, hip_stream, device);
}
int lw_poseidon_hash(const void *x, const void *y, size_t n, void *out) { return hash_entry(x, y, n, out, nullptr, false); }
int lw_poseidon_hash_device(const void *d_x, const void *d_y, size_t n, void *d_out, void *hip_stream) {
    return hash_entry(d_x, d_y, n, d_out, hip_stream, true);
}

// hash_single (single = true, row_len = 1) and hash_many
static int rows_entry(const void *rows, size_t n_rows, size_t row_len, bool single, void *out, void *hip_stream, bool device) {
    const int rc = rows_check(n_rows, row_len, row_len, POSEIDON_MAX_N, "Poseidon", "elements", rows, out, device);
    if (rc || n_rows == 0) return rc;
    return tree_rows_entry<PoseidonHash>(POSEIDON_NAMES.rows, rows, n_rows, row_len, row_len, single, out, hip_stream, device);
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
static int commit_check(const void *columns, const void *nodes_or_root, uint32_t n_cols, uint64_t col_stride, uint32_t log2n, int leaf_mode,
                        bool device) {
    if (leaf_mode != LW_POSEIDON_LEAF_SINGLE && leaf_mode != LW_POSEIDON_LEAF_MANY) { set_error("bad leaf mode %d", leaf_mode); return LW_ERR_BAD_ARG; }
    if (leaf_mode == LW_POSEIDON_LEAF_SINGLE && n_cols > 1) {   // no columns at all: the refusal of tree_commit_check
        set_error("LW_POSEIDON_LEAF_SINGLE (TreePoseidon) commits one column, not %u", n_cols);
        return LW_ERR_BAD_ARG;
    }
    return tree_commit_check(columns, nodes_or_root, n_cols, col_stride, log2n, 31, device);
}
int lw_poseidon_commit_columns_device(const void *d_columns, uint32_t n_cols, uint64_t col_stride_elems, uint32_t log2n, int bit_reverse,
                                      int leaf_mode, void *d_nodes, uint8_t *out_root, void *hip_stream) {
    const int rc = commit_check(d_columns, d_nodes, n_cols, col_stride_elems, log2n, leaf_mode, true);
    if (rc) return rc;
    return tree_commit_columns_device<PoseidonHash>(POSEIDON_NAMES, d_columns, n_cols, col_stride_elems, log2n, bit_reverse,
                                                    leaf_mode == LW_POSEIDON_LEAF_SINGLE, d_nodes, out_root, hip_stream);
}
int lw_poseidon_commit_columns(const void *columns, uint32_t n_cols, uint32_t log2n, int bit_reverse, int leaf_mode, uint8_t *out_root,
                               uint8_t *out_nodes_or_null) {
    const int rc = commit_check(columns, out_root, n_cols, 0, log2n, leaf_mode, false);
    if (rc) return rc;
    return tree_commit_columns_host<PoseidonHash>(POSEIDON_NAMES, columns, n_cols, log2n, bit_reverse, leaf_mode == LW_POSEIDON_LEAF_SINGLE,
                                                  out_root, out_nodes_or_null);
}

}  // extern "C"
