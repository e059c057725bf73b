// The test seam of the group law (lw_hip_ec_pointwise_device, include/lw_hip.h): one call of pt_add, pt_add_mixed, pt_dbl,
// pt_add_quad or pt_to_affine (ec.cuh) per row, on the curve or on its isomorphic model, with the raw (X, Y, Z) written
// back.  The MSM reaches these functions only with on-curve points of pseudo-random coordinates; here a test chooses every
// coordinate, so the field products underneath (the unreduced sums of pt_add_mixed, the two-product column accumulators of
// fe_dot, the binary GCD of pt_to_affine) run at the operands that bound them.  No formula lives in this file.
#include "internal.h"
#include "ec.cuh"

namespace lw {

constexpr int ECP_THREADS = 128;

// one work-item per row
template <class C, int OP>
__global__ __launch_bounds__(ECP_THREADS) void ec_pointwise_kernel(const void *a, const void *b, uint64_t n, void *out) {
    using B = typename C::B;
    constexpr size_t PBY = 3 * B::BYTES;
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const Point<C> p = pt_load<C>((const char *)a + i * PBY);
    Point<C> r;
    if constexpr (OP == LW_EC_OP_ADD) {
        r = pt_add<C>(p, pt_load<C>((const char *)b + i * PBY));
    } else if constexpr (OP == LW_EC_OP_ADD_MIXED) {
        const AffPoint<C> q = aff_load<C>((const char *)b + i * (2 * B::BYTES));
        r = p;
        if (!aff_is_identity<C>(q)) r = pt_add_mixed<C>(p, q);   // as the accumulation does (msm_core.cuh)
    } else if constexpr (OP == LW_EC_OP_DBL) {
        r = pt_dbl<C>(p);
    } else {
        r = pt_to_affine<C>(p);
    }
    pt_store<C>((char *)out + i * PBY, r);
}

// four lanes per row: lane s of a quad loads, keeps and stores coordinate s only, lane 3 mirrors lane 0
// (msm_group_sum_quad_kernel).  Quads are never split: the four lanes of a row past the end leave together.
template <class C>
__global__ __launch_bounds__(ECP_THREADS) void ec_pointwise_quad_kernel(const void *a, const void *b, uint64_t n, void *out) {
    using B = typename C::B;
    using T = typename B::T;
    constexpr size_t PBY = 3 * B::BYTES;
    static_assert(ECP_THREADS % 4 == 0, "quads must not straddle a workgroup");
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t i = t >> 2;
    if (i >= n) return;
    const uint32_t s = (t & 3) == 3 ? 0u : (uint32_t)(t & 3);
    const size_t off = i * PBY + s * B::BYTES;
    const T x = B::load((const char *)a + off), y = B::load((const char *)b + off);
    const T r = pt_add_quad<C>(x, y, s);
    if ((t & 3) != 3) B::store((char *)out + off, r);
}

template <class C>
static int ec_pointwise_launch(Context &c, hipStream_t stream, lw_ec_op_t op, const void *d_a, const void *d_b, uint64_t n, void *d_out) {
    const uint64_t lanes = op == LW_EC_OP_ADD_QUAD ? 4 * n : n;
    const dim3 grid((uint32_t)((lanes + ECP_THREADS - 1) / ECP_THREADS)), block(ECP_THREADS);
    hipEvent_t pe = c.prof_begin(stream);
    switch (op) {
        case LW_EC_OP_ADD: hipLaunchKernelGGL((ec_pointwise_kernel<C, LW_EC_OP_ADD>), grid, block, 0, stream, d_a, d_b, n, d_out); break;
        case LW_EC_OP_ADD_MIXED: hipLaunchKernelGGL((ec_pointwise_kernel<C, LW_EC_OP_ADD_MIXED>), grid, block, 0, stream, d_a, d_b, n, d_out); break;
        case LW_EC_OP_DBL: hipLaunchKernelGGL((ec_pointwise_kernel<C, LW_EC_OP_DBL>), grid, block, 0, stream, d_a, d_b, n, d_out); break;
        case LW_EC_OP_ADD_QUAD: hipLaunchKernelGGL((ec_pointwise_quad_kernel<C>), grid, block, 0, stream, d_a, d_b, n, d_out); break;
        default: hipLaunchKernelGGL((ec_pointwise_kernel<C, LW_EC_OP_TO_AFFINE>), grid, block, 0, stream, d_a, d_b, n, d_out); break;
    }
    c.prof_end("ec_pointwise_kernel", pe, stream);
    LW_HIP_CHECK(hipGetLastError(), LW_ERR_LAUNCH);
    return LW_OK;
}

template <class C>
static int ec_pointwise_model(Context &c, hipStream_t stream, int model, lw_ec_op_t op, const void *d_a, const void *d_b, uint64_t n,
                              void *d_out) {
    if (model == 0) return ec_pointwise_launch<C>(c, stream, op, d_a, d_b, n, d_out);
    if constexpr (IsoOf<C>::has) return ec_pointwise_launch<typename IsoOf<C>::type>(c, stream, op, d_a, d_b, n, d_out);
    return LW_ERR_BAD_ARG;   // refused by the entry point's checks
}

}  // namespace lw

using namespace lw;

extern "C" {

int lw_hip_ec_pointwise_device(lw_curve_t curve, int model, lw_ec_op_t op, const void *d_a, const void *d_b, size_t n, void *d_out,
                               void *hip_stream) {
    bool has_iso;
    switch (curve) {
        case LW_CURVE_BLS12_381_G1: has_iso = IsoOf<Bls12381G1>::has; break;
        case LW_CURVE_BN254_G1: has_iso = IsoOf<Bn254G1>::has; break;
        case LW_CURVE_BN254_G2: has_iso = IsoOf<Bn254G2>::has; break;
        case LW_CURVE_BLS12_381_G2: has_iso = IsoOf<Bls12381G2>::has; break;
        default: set_error("bad curve %d", (int)curve); return LW_ERR_BAD_ARG;
    }
    if ((int)op < (int)LW_EC_OP_ADD || (int)op > (int)LW_EC_OP_TO_AFFINE) { set_error("bad group-law op %d", (int)op); return LW_ERR_BAD_ARG; }
    if (model != 0 && !(model == 1 && has_iso)) { set_error("curve %d has no model %d", (int)curve, model); return LW_ERR_BAD_ARG; }
    if (n == 0) return LW_OK;
    const bool two = op == LW_EC_OP_ADD || op == LW_EC_OP_ADD_MIXED || op == LW_EC_OP_ADD_QUAD;
    if (!d_a || !d_out) { set_error("null buffer"); return LW_ERR_BAD_ARG; }
    if (two != (d_b != nullptr)) { set_error("op %d %s a second operand", (int)op, two ? "needs" : "takes no"); return LW_ERR_BAD_ARG; }
    if ((((uintptr_t)d_a | (uintptr_t)d_b | (uintptr_t)d_out) & 15) != 0) { set_error("device buffers must be 16-byte aligned"); return LW_ERR_BAD_ARG; }
    if (n >> 40) { set_error("%zu rows", n); return LW_ERR_ALLOC; }
    Entry en(hip_stream);
    if (en.rc) return en.rc;
    switch (curve) {
        case LW_CURVE_BLS12_381_G1: return ec_pointwise_model<Bls12381G1>(en.c, en.stream, model, op, d_a, d_b, n, d_out);
        case LW_CURVE_BN254_G1: return ec_pointwise_model<Bn254G1>(en.c, en.stream, model, op, d_a, d_b, n, d_out);
        case LW_CURVE_BN254_G2: return ec_pointwise_model<Bn254G2>(en.c, en.stream, model, op, d_a, d_b, n, d_out);
        default: return ec_pointwise_model<Bls12381G2>(en.c, en.stream, model, op, d_a, d_b, n, d_out);
    }
}

}  // extern "C"
