// Starknet Pedersen hash on the device: batched hashes and the 2-to-1 Merkle tree over leaf values that Starknet's
// Pedersen trees are.  The group law, the tables and the hash of one pair are in pedersen.cuh.
//
// Here: the hash policy PedersenHash for hash_tree.cuh (its pair kernel is the flat batched hash, one hash per
// work-item), the test seam of the group law (pedersen_add_affine_kernel), the table upload and the exported entry
// points.  The reference has no Pedersen Merkle backend: the tree is its MerkleTree (crypto/src/merkle_tree/merkle.rs)
// with hash_new_parent = PedersenStarkCurve::hash and identity leaves (hash_data = the element itself), nodes root first
// (utils.rs:43-71), so merkle.open_trees_device reads them as they are.
#include <mutex>
#include "hash_tree.cuh"
#include "pedersen.cuh"

namespace lw {

static const void *pedersen_host_table() {   // generated once per process
    alignas(16) static char table[PEDERSEN_TABLE_BYTES];
    static std::once_flag once;
    std::call_once(once, [] { pedersen_fill_table(table); });
    return table;
}

struct PedersenHash {   // the policy of hash_tree.cuh: an element and a digest are one Stark252 element
    static constexpr uint64_t DIGEST_BYTES = 32, ELEM_BYTES = 32;
    static int ready(Context &c) {   // parent reads PEDERSEN_TABLE
        return table_once(c, shared_state().pedersen_table_ready, PEDERSEN_TABLE, pedersen_host_table(), PEDERSEN_TABLE_BYTES);
    }
    static __device__ __forceinline__ void parent(const char *x, const char *y, char *out) {
        fe_store<Stark252>(out, pedersen_hash(fe_load<Stark252>(x), fe_load<Stark252>(y), PEDERSEN_TABLE));
    }
    // a leaf is its element (len = 1, checked by the entry points)
    static __device__ __forceinline__ void row(const char *row, uint32_t len, uint64_t elem_stride, int mode, char *out) {
        fe_store<Stark252>(out, fe_load<Stark252>(row));
    }
};
static constexpr TreeNames PEDERSEN_NAMES = {"pedersen_leaf_kernel", "pedersen_pair_kernel", "pedersen_top_kernel"};

// Test seam of the group law: row i lifts the affine p[i] ((0, 0): infinity) to Jacobian coordinates, rescales them by
// z[i] != 0 ((X, Y, Z) -> (X z^2, Y z^3, Z z), the same point), adds the affine q[i] with ped_add_affine and normalises
// with ped_to_affine: the two functions of the hash, so every branch of the law can be reached with chosen operands.
__global__ __launch_bounds__(256) void pedersen_add_affine_kernel(const char *p, const char *z, const char *q, uint64_t n, char *out) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const PedAffine a = ped_load_affine(p + i * 64);
    const SFe s = fe_load<Stark252>(z + i * 32);
    const SFe s2 = fe_sqr<Stark252>(s);
    const bool inf = a.x.is_zero() && a.y.is_zero();
    PedJac acc;
    acc.x = fe_mul<Stark252>(inf ? SFe::one() : a.x, s2);
    acc.y = fe_mul<Stark252>(inf ? SFe::one() : a.y, fe_mul<Stark252>(s, s2));
    acc.z = inf ? SFe::zero() : s;
    const PedAffine r = ped_to_affine(ped_add_affine(acc, ped_load_affine(q + i * 64)));
    fe_store<Stark252>(out + i * 64, r.x);
    fe_store<Stark252>(out + i * 64 + 32, r.y);
}

static constexpr uint64_t PEDERSEN_MAX_N = (uint64_t)1 << 36;   // the grid's block index stays below 2^31

}  // namespace lw

using namespace lw;

extern "C" {

int lw_pedersen_table(void *out) {
    if (!out) { set_error("null buffer"); return LW_ERR_BAD_ARG; }
    memcpy(out, pedersen_host_table(), PEDERSEN_TABLE_BYTES);
    return LW_OK;
}

static int hash_entry(const void *x, const void *y, size_t n, void *out, void *hip_stream, bool device) {
    const int rc = flat_check(n, PEDERSEN_MAX_N, "Pedersen", {x, y, out}, device);
    if (rc || n == 0) return rc;
    return tree_pair_entry<PedersenHash>(PEDERSEN_NAMES.pair, x, y, n, out, hip_stream, device);
}
int lw_pedersen_hash(const void *x, const void *y, size_t n, void *out) { return hash_entry(x, y, n, out, nullptr, false); }
int lw_pedersen_hash_device(const void *d_x, const void *d_y, size_t n, void *d_out, void *hip_stream) {
    return hash_entry(d_x, d_y, n, d_out, hip_stream, true);
}

int lw_pedersen_add_affine_device(const void *d_p, const void *d_z, const void *d_q, size_t n, void *d_out, void *hip_stream) {
    const int rc = flat_check(n, PEDERSEN_MAX_N, "Pedersen", {d_p, d_z, d_q, d_out}, true);
    if (rc || n == 0) return rc;
    Entry en(hip_stream);
    if (en.rc) return en.rc;
    return launch_1d(en.c, "pedersen_add_affine_kernel", pedersen_add_affine_kernel, blocks_for(n), en.stream, d_p, d_z, d_q, n, d_out);
}

// checks of both commitment forms; nodes_or_root: d_nodes (device form) or out_root (host form)
static int commit_check(const void *leaves, const void *nodes_or_root, uint32_t n_cols, uint32_t log2n, bool device) {
    if (!leaves || !nodes_or_root) { set_error("null buffer"); return LW_ERR_BAD_ARG; }
    if (n_cols != 1) { set_error("a Pedersen tree commits one column of leaf values, not %u", n_cols); return LW_ERR_BAD_ARG; }
    return tree_commit_check(leaves, nodes_or_root, 1, 0, log2n, 31, device);
}
int lw_pedersen_commit_leaves_device(const void *d_leaves, uint32_t n_cols, uint32_t log2n, int bit_reverse, void *d_nodes, uint8_t *out_root,
                                     void *hip_stream) {
    const int rc = commit_check(d_leaves, d_nodes, n_cols, log2n, true);
    if (rc) return rc;
    return tree_commit_columns_device<PedersenHash>(PEDERSEN_NAMES, d_leaves, 1, 0, log2n, bit_reverse, 0, d_nodes, out_root, hip_stream);
}
int lw_pedersen_commit_leaves(const void *leaves, uint32_t n_cols, uint32_t log2n, int bit_reverse, uint8_t *out_root, uint8_t *out_nodes_or_null) {
    const int rc = commit_check(leaves, out_root, n_cols, log2n, false);
    if (rc) return rc;
    return tree_commit_columns_host<PedersenHash>(PEDERSEN_NAMES, leaves, 1, log2n, bit_reverse, 0, out_root, out_nodes_or_null);
}

}  // extern "C"
