// The test seam of the field arithmetic (lw_hip_field_pointwise_device, include/lw_hip.h): one primitive of field.cuh per
// row, chosen by field_pointwise_ops.cuh, with the returned limbs written back.  The transforms, hashes and provers reach
// these primitives with pseudo-random data only; here a test chooses every operand, so the Montgomery columns (the fused
// Stark252 chains with and without the a < p bound, their scalar-operand form, the generic fips_col path of the other
// fields), the quotient estimate of fe_reduce_full and the raw add / subtract chains run at the operands that bound them.
// No arithmetic lives in this file.
#include "internal.h"
#include "field_pointwise_ops.cuh"

namespace lw {

constexpr int FPW_THREADS = 128;

// one work-item per row; a row is read completely before its result is stored, so out may be a or b where the rows are
// equally long
template <class F, int OP>
__global__ __launch_bounds__(FPW_THREADS) void field_pointwise_kernel(const void *a, const void *b, uint64_t n, void *out) {
    constexpr size_t EB = 4 * F::N;
    constexpr int ROW = fpw_row_elems(OP);
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    Fe<F> ar[ROW], br[ROW];
#pragma unroll
    for (int q = 0; q < ROW; q++) {
        // MUL_LAZY_UNIFORM: every work-item reads row 0, through the kernel argument alone (as the NTT's wave-uniform twiddle)
        if constexpr (OP == LW_FIELD_OP_MUL_LAZY_UNIFORM) ar[q] = fe_load<F>(a);
        else ar[q] = fe_load<F>((const char *)a + (i * ROW + q) * EB);
        if constexpr (fpw_two_operands(OP)) br[q] = fe_load<F>((const char *)b + (i * ROW + q) * EB);
    }
    const Fe<F> r = fe_pointwise<F, OP>(ar, br);
    fe_store<F>((char *)out + i * EB, r);
}

template <int OP>
__global__ __launch_bounds__(FPW_THREADS) void bb_pointwise_kernel(const void *a, const void *b, uint64_t n, void *out) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint64_t x, y = 0;
    if constexpr (bb_in_bytes(OP) == 8) x = ((const uint64_t *)a)[i];
    else x = ((const uint32_t *)a)[i];
    if constexpr (fpw_two_operands(OP)) y = ((const uint32_t *)b)[i];
    const uint64_t r = bb_pointwise<OP>(x, y);
    if constexpr (bb_out_bytes(OP) == 8) ((uint64_t *)out)[i] = r;
    else ((uint32_t *)out)[i] = (uint32_t)r;
}

// F has op (walks the op table from OP upwards)
template <class F, int OP = LW_FIELD_OP_ADD>
static bool fpw_field_has(int op) {
    if constexpr (OP > LW_FIELD_OP_INV) return false;
    else return op == OP ? fpw_has_op<F, OP>() : fpw_field_has<F, OP + 1>(op);
}
template <class F, int OP = LW_FIELD_OP_ADD>
static void fpw_launch(int op, dim3 grid, hipStream_t stream, const void *d_a, const void *d_b, uint64_t n, void *d_out) {
    if constexpr (OP <= LW_FIELD_OP_INV) {
        if (op != OP) return fpw_launch<F, OP + 1>(op, grid, stream, d_a, d_b, n, d_out);
        if constexpr (fpw_has_op<F, OP>())
            hipLaunchKernelGGL((field_pointwise_kernel<F, OP>), grid, dim3(FPW_THREADS), 0, stream, d_a, d_b, n, d_out);
    }
}
template <int OP = LW_FIELD_OP_ADD>
static void bb_launch(int op, dim3 grid, hipStream_t stream, const void *d_a, const void *d_b, uint64_t n, void *d_out) {
    if constexpr (OP <= LW_FIELD_OP_TO_R64) {
        if (op != OP) return bb_launch<OP + 1>(op, grid, stream, d_a, d_b, n, d_out);
        if constexpr (bb_has_op(OP))
            hipLaunchKernelGGL((bb_pointwise_kernel<OP>), grid, dim3(FPW_THREADS), 0, stream, d_a, d_b, n, d_out);
    }
}

// [p, p + pn) and [q, q + qn) share a byte
static bool fpw_overlap(const void *p, size_t pn, const void *q, size_t qn) {
    const uintptr_t a = (uintptr_t)p, b = (uintptr_t)q;
    return a < b + qn && b < a + pn;
}

}  // namespace lw

using namespace lw;

extern "C" {

int lw_hip_field_pointwise_device(lw_pw_field_t field, lw_field_op_t op, const void *d_a, const void *d_b, size_t n, void *d_out,
                                  void *hip_stream) {
    bool has;
    size_t elem = 32;   // bytes of one multi-limb element
    switch (field) {
        case LW_PW_FIELD_STARK252: has = fpw_field_has<Stark252>((int)op); break;
        case LW_PW_FIELD_FR381: has = fpw_field_has<Fr381>((int)op); break;
        case LW_PW_FIELD_FR254: has = fpw_field_has<Fr254>((int)op); break;
        case LW_PW_FIELD_FP381: has = fpw_field_has<Fp381>((int)op); elem = 48; break;
        case LW_PW_FIELD_FP254: has = fpw_field_has<Fp254>((int)op); break;
        case LW_PW_FIELD_BABYBEAR: has = bb_has_op((int)op); break;
        default: set_error("bad pointwise field %d", (int)field); return LW_ERR_BAD_ARG;
    }
    if (!has) { set_error("pointwise field %d has no op %d", (int)field, (int)op); return LW_ERR_BAD_ARG; }
    if (n == 0) return LW_OK;
    const bool two = fpw_two_operands((int)op), bb = field == LW_PW_FIELD_BABYBEAR;
    if (!d_a || !d_out) { set_error("null buffer"); return LW_ERR_BAD_ARG; }
    if (two != (d_b != nullptr)) { set_error("op %d %s a second operand", (int)op, two ? "needs" : "takes no"); return LW_ERR_BAD_ARG; }
    if ((((uintptr_t)d_a | (uintptr_t)d_b | (uintptr_t)d_out) & 15) != 0) { set_error("device buffers must be 16-byte aligned"); return LW_ERR_BAD_ARG; }
    if (n >> 40) { set_error("%zu rows", n); return LW_ERR_ALLOC; }
    // bytes per row of an operand and of the output; the output may be an operand only row for row
    const size_t in_row = bb ? (size_t)bb_in_bytes((int)op) : elem * fpw_row_elems((int)op);
    const size_t b_row = bb ? 4 : in_row;
    const size_t out_row = bb ? (size_t)bb_out_bytes((int)op) : elem;
    const bool uniform = op == LW_FIELD_OP_MUL_LAZY_UNIFORM;
    if (fpw_overlap(d_a, uniform ? in_row : n * in_row, d_out, n * out_row) && (uniform || d_a != d_out || in_row != out_row)) {
        set_error("d_out overlaps d_a"); return LW_ERR_BAD_ARG;
    }
    if (two && fpw_overlap(d_b, n * b_row, d_out, n * out_row) && (d_b != d_out || b_row != out_row)) {
        set_error("d_out overlaps d_b"); return LW_ERR_BAD_ARG;
    }
    Entry en(hip_stream);
    if (en.rc) return en.rc;
    const dim3 grid((uint32_t)((n + FPW_THREADS - 1) / FPW_THREADS));
    hipEvent_t pe = en.c.prof_begin(en.stream);
    switch (field) {
        case LW_PW_FIELD_STARK252: fpw_launch<Stark252>((int)op, grid, en.stream, d_a, d_b, n, d_out); break;
        case LW_PW_FIELD_FR381: fpw_launch<Fr381>((int)op, grid, en.stream, d_a, d_b, n, d_out); break;
        case LW_PW_FIELD_FR254: fpw_launch<Fr254>((int)op, grid, en.stream, d_a, d_b, n, d_out); break;
        case LW_PW_FIELD_FP381: fpw_launch<Fp381>((int)op, grid, en.stream, d_a, d_b, n, d_out); break;
        case LW_PW_FIELD_FP254: fpw_launch<Fp254>((int)op, grid, en.stream, d_a, d_b, n, d_out); break;
        default: bb_launch((int)op, grid, en.stream, d_a, d_b, n, d_out); break;
    }
    en.c.prof_end("field_pointwise_kernel", pe, en.stream);
    LW_HIP_CHECK(hipGetLastError(), LW_ERR_LAUNCH);
    return LW_OK;
}

}  // extern "C"
