// The op table of the field-arithmetic seam (csrc/field_pointwise_ops.cuh) on the host: the same fe_pointwise / bb_pointwise
// the device kernel calls, over the rows of a vector file.  tests/test_field_pointwise_cpu.py builds this with g++ under
// AddressSanitizer and UBSan and compares every result with Python integers, which runs the shared non-asm code of
// field.cuh (carry chains, reduce_once, fe_reduce_full, fe_cond_sub_kp, the raw adds, the host products, bb_*) at every
// chosen operand.  A plain program: no device, no preloaded runtime.
//
// usage: field_pointwise_host IN OUT
// IN:  jobs until the end of the file: u32 field (lw_pw_field_t), u32 op (lw_field_op_t), u64 n, then the n rows of a and,
//      for an op with two operands, the n rows of b, in the layout of the entry point (MUL_LAZY_UNIFORM: one row of a).
// OUT: the n result rows of every job, back to back.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>
struct uint4 { unsigned x, y, z, w; };
static inline uint4 make_uint4(unsigned a, unsigned b, unsigned c, unsigned d) { return uint4{a, b, c, d}; }
#include "../lambda_elliptic_curves_amd/csrc/field_pointwise_ops.cuh"
using namespace lw;

static bool read_rows(FILE *f, uint4 *&dst, std::vector<uint4> &store, size_t bytes) {
    store.assign((bytes + 15) / 16 + 1, uint4{0, 0, 0, 0});   // 16-byte aligned, as the device buffers are
    dst = store.data();
    return fread(dst, 1, bytes, f) == bytes;
}

template <class F, int OP = LW_FIELD_OP_ADD>
static int run_field(int op, FILE *in, FILE *out, uint64_t n) {
    if constexpr (OP > LW_FIELD_OP_INV) return 2;
    else {
        if (op != OP) return run_field<F, OP + 1>(op, in, out, n);
        if constexpr (!fpw_has_op<F, OP>()) return 2;
        else {
            constexpr size_t EB = 4 * F::N;
            constexpr int ROW = fpw_row_elems(OP);
            constexpr bool UNIFORM = OP == LW_FIELD_OP_MUL_LAZY_UNIFORM;
            std::vector<uint4> sa, sb, so;
            uint4 *a = nullptr, *b = nullptr;
            if (!read_rows(in, a, sa, (UNIFORM ? 1 : n) * ROW * EB)) return 3;
            if (fpw_two_operands(OP) && !read_rows(in, b, sb, n * ROW * EB)) return 3;
            so.assign(n * EB / 16 + 1, uint4{0, 0, 0, 0});
            for (uint64_t i = 0; i < n; i++) {
                Fe<F> ar[ROW], br[ROW];
                for (int q = 0; q < ROW; q++) {
                    ar[q] = fe_load<F>((const char *)a + (UNIFORM ? 0 : (i * ROW + q) * EB));
                    br[q] = fpw_two_operands(OP) ? fe_load<F>((const char *)b + (i * ROW + q) * EB) : Fe<F>::zero();
                }
                fe_store<F>((char *)so.data() + i * EB, fe_pointwise<F, OP>(ar, br));
            }
            return fwrite(so.data(), 1, n * EB, out) == n * EB ? 0 : 4;
        }
    }
}

template <int OP = LW_FIELD_OP_ADD>
static int run_bb(int op, FILE *in, FILE *out, uint64_t n) {
    if constexpr (OP > LW_FIELD_OP_TO_R64) return 2;
    else {
        if (op != OP) return run_bb<OP + 1>(op, in, out, n);
        if constexpr (!bb_has_op(OP)) return 2;
        else {
            std::vector<uint4> sa, sb;
            uint4 *a = nullptr, *b = nullptr;
            if (!read_rows(in, a, sa, n * bb_in_bytes(OP))) return 3;
            if (fpw_two_operands(OP) && !read_rows(in, b, sb, n * 4)) return 3;
            for (uint64_t i = 0; i < n; i++) {
                uint64_t x = 0, y = 0;
                memcpy(&x, (const char *)a + i * bb_in_bytes(OP), bb_in_bytes(OP));   // little-endian host
                if (fpw_two_operands(OP)) memcpy(&y, (const char *)b + i * 4, 4);
                const uint64_t r = bb_pointwise<OP>(x, y);
                const uint32_t r32 = (uint32_t)r;
                const size_t ob = bb_out_bytes(OP);
                if (fwrite(ob == 8 ? (const void *)&r : (const void *)&r32, 1, ob, out) != ob) return 4;
            }
            return 0;
        }
    }
}

int main(int argc, char **argv) {
    if (argc != 3) return 1;
    FILE *in = fopen(argv[1], "rb"), *out = fopen(argv[2], "wb");
    if (!in || !out) return 1;
    int jobs = 0;
    for (;;) {
        uint32_t head[2];
        uint64_t n;
        if (fread(head, 4, 2, in) != 2) break;
        if (fread(&n, 8, 1, in) != 1 || n > (1u << 24)) return 3;
        int rc;
        switch (head[0]) {
            case LW_PW_FIELD_STARK252: rc = run_field<Stark252>((int)head[1], in, out, n); break;
            case LW_PW_FIELD_FR381: rc = run_field<Fr381>((int)head[1], in, out, n); break;
            case LW_PW_FIELD_FR254: rc = run_field<Fr254>((int)head[1], in, out, n); break;
            case LW_PW_FIELD_FP381: rc = run_field<Fp381>((int)head[1], in, out, n); break;
            case LW_PW_FIELD_FP254: rc = run_field<Fp254>((int)head[1], in, out, n); break;
            case LW_PW_FIELD_BABYBEAR: rc = run_bb((int)head[1], in, out, n); break;
            default: rc = 2;
        }
        if (rc) {
            fprintf(stderr, "job %d (field %u, op %u): error %d\n", jobs, head[0], head[1], rc);
            return rc;
        }
        jobs++;
    }
    if (fclose(out) != 0) return 4;
    printf("ok %d\n", jobs);
    return 0;
}
