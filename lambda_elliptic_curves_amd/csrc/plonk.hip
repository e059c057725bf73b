// PLONK prover rounds 1-3 on the device (provers/plonk/src/prover.rs:311-535, without the commitments): the wire
// polynomials, the permutation grand product z and the quotient t, computed between the library's own NTT kernels with
// nothing but challenges and blinders coming from the host.  DESIGN §4.8 has the data flow.
//
// The circuit handle (lw_plonk_circuit_t) is the device-side CommonPreprocessedInput (provers/plonk/src/setup.rs): it
// keeps what does not change from proof to proof — the nine coset evaluations round 3 reads (ql qr qo qm qc s1 s2 s3 and
// l1 on k1 * <w_4n>), the table x_i = k1 * w_4n^i, the three s_lagrange columns — and the few constants that have closed
// forms: on the coset X^n takes the four values k1^n * i4^j (i4 = w_4n^n), so Z_H = X^n - 1 takes four values too, whose
// inverses are computed once on the host.
//
// Round 2 is a prefix product.  z_i = prod_{j<i} num_j / den_j needs no division per row: with N_i the exclusive prefix
// product of num, S_i = prod_{i <= j <= n-2} den_j the suffix product of den and T = 1 / prod_{j <= n-2} den_j,
//     z_i = N_i * S_i * T,
// one inversion per call (on the host, from the 32 bytes that also decide LW_ERR_INV_ZERO).  The scans are
// reduce-then-scan over three separate launches, whatever n — no workgroup waits for another one:
//   1. plonk_z_reduce_kernel   every tile of PLONK_TILE rows computes num_i, den_i and their two products
//   2. plonk_z_carry_kernel    ONE workgroup of PLONK_TOP threads scans the tile products: thread r owns
//                              ceil(tiles / PLONK_TOP) consecutive tiles; out come the product of all num tiles before a
//                              tile, of all den tiles after it, and the total den product
//   3. plonk_z_rescan_kernel   every tile recomputes its rows, scans them with its two carries and stores z
// Rows n-1 and beyond count as num = den = 1: the reference's loop stops at n-2 (prover.rs:358).
//
// Every stored value is fully reduced: fe_add / fe_sub / fe_mul return canonical residues for canonical operands in both
// fields (Stark252's lazy range belongs to the NTT butterflies only), so the results are the reference's bit for bit.
#include <string.h>
#include <new>
#include "internal.h"
#include "ntt_kernels.cuh"

namespace lw {

constexpr int PLONK_THREADS = 256;
constexpr int PLONK_E = 2;                                             // consecutive rows per thread
constexpr uint64_t PLONK_TILE = (uint64_t)PLONK_THREADS * PLONK_E;    // 512 rows per workgroup
constexpr int PLONK_TOP = 64;                                          // threads of the carry kernel
constexpr int PLONK_NCOL = 9;                                          // ql qr qo qm qc s1 s2 s3 l1

template <class F>
__device__ __forceinline__ Fe<F> ld(const uint4 *p, uint64_t i) { return unpack_mem<F>(p[2 * i], p[2 * i + 1]); }
template <class F>
__device__ __forceinline__ void st(uint4 *p, uint64_t i, const Fe<F> &v) {
    uint4 q0, q1;
    pack_mem<F>(v, q0, q1);
    p[2 * i] = q0;
    p[2 * i + 1] = q1;
}

// Hillis-Steele scan of products over the workgroup's T threads: on return v (and lds[r]) is the product over r' <= r
// (SUFFIX: r' >= r).  The caller synchronises before it reuses lds.
template <class F, bool SUFFIX, int T>
__device__ __forceinline__ Fe<F> block_scan_mul(Fe<F> v, Fe<F> *lds) {
    const int r = threadIdx.x;
#pragma unroll 1
    for (int d = 1; d < T; d <<= 1) {
        lds[r] = v;
        __syncthreads();
        const int o = SUFFIX ? r + d : r - d;
        if (o >= 0 && o < T) v = fe_mul<F>(v, lds[o]);
        __syncthreads();
    }
    lds[r] = v;
    __syncthreads();
    return v;
}
// the neighbour's inclusive value = this thread's exclusive one
template <class F, bool SUFFIX, int T>
__device__ __forceinline__ Fe<F> scan_exclusive(const Fe<F> *lds) {
    const int o = SUFFIX ? (int)threadIdx.x + 1 : (int)threadIdx.x - 1;
    return (o >= 0 && o < T) ? lds[o] : Fe<F>::one();
}

// ---------------------------------------------------------------- round 2: the grand product
template <class F>
struct PlonkZArgs {
    const uint4 *w;         // witness a | b | c, n rows each
    const uint4 *sl;        // s1_lagrange | s2_lagrange | s3_lagrange
    const uint4 *x;         // x_i = k1 * w_4n^i: the domain element w_n^i is x_{4i} / k1
    uint4 *tile_num, *tile_den, *carry_num, *carry_den, *total;
    uint4 *z;
    uint64_t n, ntiles;
    Fe<F> beta, gamma;
    Fe<F> bd[3];            // beta / k1, beta, beta * k1: times x_{4i} they are beta * w^i * {1, k1, k1^2}
    Fe<F> t;                // 1 / (product of den over rows 0 .. n-2)  (rescan)
};

// num_i and den_i of prover.rs:360-363; rows the loop never reaches count as 1
template <class F>
__device__ __forceinline__ void plonk_num_den(const PlonkZArgs<F> &a, uint64_t i, Fe<F> &num, Fe<F> &den) {
    if (i + 1 >= a.n) {
        num = den = Fe<F>::one();
        return;
    }
    const Fe<F> x = ld<F>(a.x, 4 * i);
    const Fe<F> ag = fe_add<F>(ld<F>(a.w, i), a.gamma), bg = fe_add<F>(ld<F>(a.w, a.n + i), a.gamma),
                cg = fe_add<F>(ld<F>(a.w, 2 * a.n + i), a.gamma);
    num = fe_mul<F>(fe_mul<F>(fe_add<F>(ag, fe_mul<F>(x, a.bd[0])), fe_add<F>(bg, fe_mul<F>(x, a.bd[1]))),
                    fe_add<F>(cg, fe_mul<F>(x, a.bd[2])));
    den = fe_mul<F>(fe_mul<F>(fe_add<F>(ag, fe_mul<F>(ld<F>(a.sl, i), a.beta)), fe_add<F>(bg, fe_mul<F>(ld<F>(a.sl, a.n + i), a.beta))),
                    fe_add<F>(cg, fe_mul<F>(ld<F>(a.sl, 2 * a.n + i), a.beta)));
}

template <class F>
__global__ __launch_bounds__(PLONK_THREADS) void plonk_z_reduce_kernel(const PlonkZArgs<F> a) {
    __shared__ Fe<F> lds[2][PLONK_THREADS];
    const int r = threadIdx.x;
    const uint64_t base = (uint64_t)blockIdx.x * PLONK_TILE + (uint64_t)r * PLONK_E;
    Fe<F> pn = Fe<F>::one(), pd = Fe<F>::one();
#pragma unroll
    for (int e = 0; e < PLONK_E; e++) {
        Fe<F> num, den;
        plonk_num_den<F>(a, base + e, num, den);
        pn = fe_mul<F>(pn, num);
        pd = fe_mul<F>(pd, den);
    }
#pragma unroll 1
    for (int s = PLONK_THREADS / 2; s >= 1; s >>= 1) {
        lds[0][r] = pn;
        lds[1][r] = pd;
        __syncthreads();
        if (r < s) {
            pn = fe_mul<F>(pn, lds[0][r + s]);
            pd = fe_mul<F>(pd, lds[1][r + s]);
        }
        __syncthreads();
    }
    if (r == 0) {
        st<F>(a.tile_num, blockIdx.x, pn);
        st<F>(a.tile_den, blockIdx.x, pd);
    }
}

template <class F>
__global__ __launch_bounds__(PLONK_TOP) void plonk_z_carry_kernel(const PlonkZArgs<F> a) {
    __shared__ Fe<F> lds[PLONK_TOP];
    const uint64_t g = (a.ntiles + PLONK_TOP - 1) / PLONK_TOP;
    const uint64_t t0 = (uint64_t)threadIdx.x * g;
    const uint64_t t1 = t0 + g < a.ntiles ? t0 + g : a.ntiles;   // t0 >= t1: this thread owns no tile
    Fe<F> pn = Fe<F>::one(), pd = Fe<F>::one();
    for (uint64_t t = t0; t < t1; t++) {
        pn = fe_mul<F>(pn, ld<F>(a.tile_num, t));
        pd = fe_mul<F>(pd, ld<F>(a.tile_den, t));
    }
    block_scan_mul<F, false, PLONK_TOP>(pn, lds);
    Fe<F> carry = scan_exclusive<F, false, PLONK_TOP>(lds);
    __syncthreads();
    for (uint64_t t = t0; t < t1; t++) {
        st<F>(a.carry_num, t, carry);
        carry = fe_mul<F>(carry, ld<F>(a.tile_num, t));
    }
    const Fe<F> all = block_scan_mul<F, true, PLONK_TOP>(pd, lds);
    carry = scan_exclusive<F, true, PLONK_TOP>(lds);
    for (uint64_t t = t1; t > t0; t--) {
        st<F>(a.carry_den, t - 1, carry);
        carry = fe_mul<F>(carry, ld<F>(a.tile_den, t - 1));
    }
    if (threadIdx.x == 0) st<F>(a.total, 0, all);
}

template <class F>
__global__ __launch_bounds__(PLONK_THREADS) void plonk_z_rescan_kernel(const PlonkZArgs<F> a) {
    __shared__ Fe<F> lds[PLONK_THREADS];
    static_assert(PLONK_E == 2, "the two rows of a thread are written out below");
    const uint64_t base = (uint64_t)blockIdx.x * PLONK_TILE + (uint64_t)threadIdx.x * PLONK_E;
    Fe<F> n0, d0, n1, d1;
    plonk_num_den<F>(a, base, n0, d0);
    plonk_num_den<F>(a, base + 1, n1, d1);
    block_scan_mul<F, false, PLONK_THREADS>(fe_mul<F>(n0, n1), lds);
    const Fe<F> before = fe_mul<F>(fe_mul<F>(scan_exclusive<F, false, PLONK_THREADS>(lds), ld<F>(a.carry_num, blockIdx.x)), a.t);
    __syncthreads();
    block_scan_mul<F, true, PLONK_THREADS>(fe_mul<F>(d0, d1), lds);
    const Fe<F> after = fe_mul<F>(scan_exclusive<F, true, PLONK_THREADS>(lds), ld<F>(a.carry_den, blockIdx.x));
    // z_i = T * N_i * S_i:  N_{i+1} = N_i num_i,  S_i = den_i S_{i+1}
    const Fe<F> s1 = fe_mul<F>(d1, after);
    if (base < a.n) st<F>(a.z, base, fe_mul<F>(before, fe_mul<F>(d0, s1)));
    if (base + 1 < a.n) st<F>(a.z, base + 1, fe_mul<F>(fe_mul<F>(before, n0), s1));
}

// ---------------------------------------------------------------- blinding (rounds 1 and 2)
// out = p + (b_0 + b_1 X [+ b_2 X^2]) (X^n - 1), stated as accumulation so that any n >= 1 is right:
// out[i] -= b_i, out[n + i] += b_i.  src: `batch` dense blocks of n coefficients; dst: blocks of n + nb.
template <class F>
struct PlonkBlindArgs {
    const uint4 *src;
    uint4 *dst;
    uint64_t n;
    uint32_t nb;
    Fe<F> b[6];   // [block * nb + i]; zero without blinders
};
template <class F>
__global__ __launch_bounds__(PLONK_THREADS) void plonk_blind_kernel(const PlonkBlindArgs<F> a) {
    const uint64_t j = (uint64_t)blockIdx.x * PLONK_THREADS + threadIdx.x;
    if (j >= a.n + a.nb) return;
    const uint32_t k = blockIdx.y;
    Fe<F> v = j < a.n ? ld<F>(a.src, k * a.n + j) : Fe<F>::zero();
    for (uint32_t i = 0; i < a.nb; i++) {
        if (j == i) v = fe_sub<F>(v, a.b[k * a.nb + i]);
        if (j == a.n + i) v = fe_add<F>(v, a.b[k * a.nb + i]);
    }
    st<F>(a.dst, k * (a.n + a.nb) + j, v);
}

// ---------------------------------------------------------------- round 3: the quotient on the coset
template <class F>
struct PlonkQArgs {
    uint4 *lde;             // a | b | c | z | pi on the coset, 4n each: low-degree extensions of the n low coefficients;
                            // the quotient's evaluations are written over a
    const uint4 *cir;       // ql | qr | qo | qm | qc | s1 | s2 | s3 | l1 on the coset (the handle)
    const uint4 *x;         // x_i = k1 * w_4n^i
    const uint4 *p_abc;     // 3 x (n + 2) coefficients: the kernel reads the two high ones of each block
    const uint4 *p_z;       // n + 3 coefficients: the three high ones
    uint64_t n;
    uint32_t has_pi;
    Fe<F> beta, gamma, alpha, beta_k1, beta_k2, omega;
    Fe<F> xn[4];            // x_i^n = k1^n * i4^(i mod 4)
    Fe<F> zh_inv[4];        // 1 / (x_i^n - 1)
};

// p(x_i) of a blinded polynomial = LDE(low n coefficients)(x_i) + x_i^n * high(x_i); one thread per coset point.
// Everything of prover.rs:440-506 happens here in registers, ((p2 alpha + p1) alpha + constraints) / Z_H.
template <class F>
__global__ __launch_bounds__(PLONK_THREADS) void plonk_quotient_kernel(const PlonkQArgs<F> q) {
    const uint64_t n4 = 4 * q.n;
    const uint64_t i = (uint64_t)blockIdx.x * PLONK_THREADS + threadIdx.x;
    if (i >= n4) return;
    const Fe<F> x = ld<F>(q.x, i);
    const Fe<F> xn = q.xn[i & 3];
    const uint64_t hb = q.n + 2;
    Fe<F> w[3];
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const Fe<F> hi = fe_add<F>(fe_mul<F>(ld<F>(q.p_abc, k * hb + q.n + 1), x), ld<F>(q.p_abc, k * hb + q.n));
        w[k] = fe_add<F>(ld<F>(q.lde, k * n4 + i), fe_mul<F>(xn, hi));
    }
    const Fe<F> z0 = ld<F>(q.p_z, q.n), z1 = ld<F>(q.p_z, q.n + 1), z2 = ld<F>(q.p_z, q.n + 2);
    Fe<F> z = fe_add<F>(fe_mul<F>(fe_add<F>(fe_mul<F>(z2, x), z1), x), z0);
    z = fe_add<F>(ld<F>(q.lde, 3 * n4 + i), fe_mul<F>(xn, z));
    // z(w x_i): x_{i+4} = w_n x_i, and (w_n x_i)^n = x_i^n
    const uint64_t iw = (i + 4) & (n4 - 1);
    const Fe<F> xw = fe_mul<F>(x, q.omega);
    Fe<F> zw = fe_add<F>(fe_mul<F>(fe_add<F>(fe_mul<F>(z2, xw), z1), xw), z0);
    zw = fe_add<F>(ld<F>(q.lde, 3 * n4 + iw), fe_mul<F>(xn, zw));

    // a b qm + a ql + b qr + c qo + qc + pi
    Fe<F> acc = fe_mul<F>(fe_mul<F>(w[0], w[1]), ld<F>(q.cir, 3 * n4 + i));
    acc = fe_add<F>(acc, fe_mul<F>(w[0], ld<F>(q.cir, i)));
    acc = fe_add<F>(acc, fe_mul<F>(w[1], ld<F>(q.cir, n4 + i)));
    acc = fe_add<F>(acc, fe_mul<F>(w[2], ld<F>(q.cir, 2 * n4 + i)));
    acc = fe_add<F>(acc, ld<F>(q.cir, 4 * n4 + i));
    if (q.has_pi) acc = fe_add<F>(acc, ld<F>(q.lde, 4 * n4 + i));

    w[0] = fe_add<F>(w[0], q.gamma);
    w[1] = fe_add<F>(w[1], q.gamma);
    w[2] = fe_add<F>(w[2], q.gamma);
    Fe<F> f = fe_mul<F>(fe_add<F>(w[0], fe_mul<F>(x, q.beta)), fe_add<F>(w[1], fe_mul<F>(x, q.beta_k1)));
    f = fe_mul<F>(f, fe_add<F>(w[2], fe_mul<F>(x, q.beta_k2)));
    Fe<F> g = fe_mul<F>(fe_add<F>(w[0], fe_mul<F>(ld<F>(q.cir, 5 * n4 + i), q.beta)), fe_add<F>(w[1], fe_mul<F>(ld<F>(q.cir, 6 * n4 + i), q.beta)));
    g = fe_mul<F>(g, fe_add<F>(w[2], fe_mul<F>(ld<F>(q.cir, 7 * n4 + i), q.beta)));
    const Fe<F> p1 = fe_sub<F>(fe_mul<F>(g, zw), fe_mul<F>(f, z));
    const Fe<F> p2 = fe_mul<F>(fe_sub<F>(z, Fe<F>::one()), ld<F>(q.cir, 8 * n4 + i));
    Fe<F> p = fe_add<F>(fe_mul<F>(fe_add<F>(fe_mul<F>(p2, q.alpha), p1), q.alpha), acc);
    st<F>(q.lde, i, fe_mul<F>(p, q.zh_inv[i & 3]));
}

// t (4n coefficients, read as zero beyond) -> t_lo | t_mid | t_hi, n + 3 coefficients each (prover.rs:509-520):
// block k = t[k (n+2) .. (k+1) (n+2)) with the previous block's blinder subtracted from coefficient 0, then its own
template <class F>
struct PlonkSplitArgs {
    const uint4 *t;
    uint4 *out;
    uint64_t n;
    Fe<F> b[2];
};
template <class F>
__global__ __launch_bounds__(PLONK_THREADS) void plonk_t_split_kernel(const PlonkSplitArgs<F> a) {
    const uint64_t j = (uint64_t)blockIdx.x * PLONK_THREADS + threadIdx.x;
    const uint32_t k = blockIdx.y;
    if (j > a.n + 2) return;
    Fe<F> v = Fe<F>::zero();
    if (j < a.n + 2) {
        const uint64_t idx = k * (a.n + 2) + j;
        if (idx < 4 * a.n) v = ld<F>(a.t, idx);
        if (j == 0 && k > 0) v = fe_sub<F>(v, a.b[k - 1]);
    } else if (k < 2) {
        v = a.b[k];
    }
    st<F>(a.out, k * (a.n + 3) + j, v);
}

}  // namespace lw

// The device-side CommonPreprocessedInput.  Device bytes held: (3 + 4 * 9 + 4) * n * 32 = 1376 n
// (s_lagrange, the nine coset columns, the x table): 1.34 GiB at n = 2^20.
struct lw_plonk_circuit {
    lw_field_t field;
    size_t n;
    uint32_t log2n;
    uint64_t k1_ref[4];                          // k1 as the caller stores it (the NTT's coset argument)
    uint32_t k1[8], k1_inv[8], omega[8];         // internal words, Montgomery form
    uint32_t xn[4][8], zh_inv[4][8];
    lw::DeviceBuf s_lagrange, cols, x;
};

namespace lw {

template <class F>
static Fe<F> fe_words(const uint32_t *w) {
    Fe<F> r;
    for (int i = 0; i < 8; i++) r.v[i] = w[i];
    return r;
}
template <class F>
static Fe<F> fe_host(const void *ref) {   // one element of caller memory (8-byte aligned at best)
    alignas(16) uint64_t w[4];
    memcpy(w, ref, 32);
    return fe_load<F>(w);
}
template <class F>
static Fe<F> fe_opt(const void *elems, size_t i) {   // element i of a host vector, zero when there is none
    return elems ? fe_host<F>((const char *)elems + i * 32) : Fe<F>::zero();
}

static bool plonk_field_ok(lw_field_t f) {
    if (f == LW_FIELD_STARK252 || f == LW_FIELD_BLS12_381_FR) return true;
    set_error("field %d: the PLONK rounds take STARK252 or BLS12_381_FR (4 x u64 limbs)", (int)f);
    return false;
}
static bool aligned16(const void *p) { return ((uintptr_t)p & 15) == 0; }
static int null_arg() {
    set_error("null argument");
    return LW_ERR_BAD_ARG;
}
static int misaligned() {
    set_error("device buffers must be 16-byte aligned");
    return LW_ERR_BAD_ARG;
}

// the host-side constants of a circuit: k1^n i4^j, the inverse vanishing values, w_n
template <class F>
static int circuit_constants(lw_plonk_circuit &h, const void *k1) {
    const Fe<F> k = fe_host<F>(k1);
    if (k.is_zero()) { set_error("coset offset k1 is zero"); return LW_ERR_INV_ZERO; }
    uint32_t w4[8], wn[8];
    int rc = ntt256_root_words((int)h.field, h.log2n + 2, false, w4);
    if (rc == LW_OK) rc = ntt256_root_words((int)h.field, h.log2n, false, wn);
    if (rc) return rc;
    const Fe<F> i4 = fe_pow_u64<F>(fe_words<F>(w4), h.n);
    Fe<F> v = fe_pow_u64<F>(k, h.n);
    for (int j = 0; j < 4; j++) {
        const Fe<F> zh = fe_sub<F>(v, Fe<F>::one());
        if (zh.is_zero()) { set_error("the vanishing polynomial has a root on the coset k1 * <w_4n>"); return LW_ERR_INV_ZERO; }
        const Fe<F> zi = fe_inv<F>(zh);
        for (int i = 0; i < 8; i++) { h.xn[j][i] = v.v[i]; h.zh_inv[j][i] = zi.v[i]; }
        v = fe_mul<F>(v, i4);
    }
    const Fe<F> ki = fe_inv<F>(k);
    for (int i = 0; i < 8; i++) { h.k1[i] = k.v[i]; h.k1_inv[i] = ki.v[i]; h.omega[i] = wn[i]; }
    memcpy(h.k1_ref, k1, 32);
    return LW_OK;
}

// uploads and evaluates the circuit's polynomials: one batch of nine low-degree extensions n -> 4n on the coset
static int circuit_build(Context &c, lw_plonk_circuit &h, const void *q_coeffs, const void *s_coeffs, const void *s_lagrange, hipStream_t s) {
    const size_t n = h.n, n4 = 4 * n;
    if (h.s_lagrange.ensure(3 * n * 32) || h.cols.ensure(PLONK_NCOL * n4 * 32) || h.x.ensure(n4 * 32)) return LW_ERR_ALLOC;
    if (c.host_io_a.ensure((PLONK_NCOL * n + 1) * 32)) return LW_ERR_ALLOC;
    char *stage = (char *)c.host_io_a.p;
    LW_HIP_CHECK(hipMemcpyAsync(stage, q_coeffs, 5 * n * 32, hipMemcpyHostToDevice, s), LW_ERR_LAUNCH);
    LW_HIP_CHECK(hipMemcpyAsync(stage + 5 * n * 32, s_coeffs, 3 * n * 32, hipMemcpyHostToDevice, s), LW_ERR_LAUNCH);
    LW_HIP_CHECK(hipMemcpyAsync(h.s_lagrange.p, s_lagrange, 3 * n * 32, hipMemcpyHostToDevice, s), LW_ERR_LAUNCH);
    // l1 = interpolate_fft(1, 0, ..., 0) = (1/n) (1 + X + ... + X^(n-1))
    uint32_t ninv[8];
    alignas(16) uint64_t ninv_ref[4];
    int rc = ntt256_inv_u64_words((int)h.field, n, ninv);
    if (rc) return rc;
    for (int k = 0; k < 8; k++) ((uint32_t *)ninv_ref)[2 * (3 - k / 2) + (k & 1)] = ninv[k];
    char *d_ninv = stage + PLONK_NCOL * n * 32;
    LW_HIP_CHECK(hipMemcpyAsync(d_ninv, ninv_ref, 32, hipMemcpyHostToDevice, s), LW_ERR_LAUNCH);
    rc = broadcast_device(32, d_ninv, stage + 8 * n * 32, n, 1, n, s);
    if (rc) return rc;
    rc = ntt_device_locked(c, h.field, LW_LAYOUT_U64_LIMBS_MS_FIRST, LW_DIR_FORWARD, stage, h.cols.p, h.log2n + 2, PLONK_NCOL, 0, h.k1_ref, s,
                           h.log2n);
    if (rc) return rc;
    rc = ntt256_gen_powers((int)h.field, h.log2n + 2, n4, 0, false, h.k1, h.x.p, s);   // synchronises
    if (rc) return rc;
    LW_HIP_CHECK(hipStreamSynchronize(s), LW_ERR_LAUNCH);
    return LW_OK;
}

template <class F>
static int blind_launch(Context &c, const void *d_src, void *d_dst, uint64_t n, uint32_t batch, uint32_t nb, const void *blinders, hipStream_t s) {
    PlonkBlindArgs<F> a;
    a.src = (const uint4 *)d_src;
    a.dst = (uint4 *)d_dst;
    a.n = n;
    a.nb = nb;
    for (uint32_t i = 0; i < 6; i++) a.b[i] = i < batch * nb ? fe_opt<F>(blinders, i) : Fe<F>::zero();
    hipEvent_t pe = c.prof_begin(s);
    hipLaunchKernelGGL((plonk_blind_kernel<F>), dim3((uint32_t)((n + nb + PLONK_THREADS - 1) / PLONK_THREADS), batch), dim3(PLONK_THREADS), 0, s, a);
    c.prof_end("plonk_blind_kernel", pe, s);
    LW_HIP_CHECK(hipGetLastError(), LW_ERR_LAUNCH);
    return LW_OK;
}

// round 1 on device buffers: d_w 3 x n values, d_out 3 x (n + 2) coefficients
template <class F>
static int round1_locked(Context &c, const lw_plonk_circuit &h, const void *d_w, const void *blinders, void *d_out, hipStream_t s) {
    const size_t n = h.n;
    if (c.pipe_tmp.ensure(3 * n * 32)) return LW_ERR_ALLOC;
    int rc = ntt_device_locked(c, h.field, LW_LAYOUT_U64_LIMBS_MS_FIRST, LW_DIR_INVERSE, d_w, c.pipe_tmp.p, h.log2n, 3, 0, nullptr, s);
    if (rc) return rc;
    return blind_launch<F>(c, c.pipe_tmp.p, d_out, n, 3, 2, blinders, s);
}

// round 2 on device buffers; synchronises once (the den product decides LW_ERR_INV_ZERO and is inverted on the host)
template <class F>
static int round2_locked(Context &c, const lw_plonk_circuit &h, const void *d_w, const void *beta, const void *gamma, const void *blinders,
                         void *d_z_or_null, void *d_out, hipStream_t s) {
    const size_t n = h.n;
    const uint64_t nt = (n + PLONK_TILE - 1) / PLONK_TILE;
    // [z n | coefficients n | tile_num | tile_den | carry_num | carry_den (nt each) | total]
    if (c.pipe_tmp.ensure((2 * n + 4 * nt + 1) * 32)) return LW_ERR_ALLOC;
    uint4 *ws = (uint4 *)c.pipe_tmp.p;
    PlonkZArgs<F> a;
    a.w = (const uint4 *)d_w;
    a.sl = (const uint4 *)h.s_lagrange.p;
    a.x = (const uint4 *)h.x.p;
    a.z = d_z_or_null ? (uint4 *)d_z_or_null : ws;
    uint4 *coef = ws + 2 * n;
    a.tile_num = ws + 4 * n;
    a.tile_den = a.tile_num + 2 * nt;
    a.carry_num = a.tile_den + 2 * nt;
    a.carry_den = a.carry_num + 2 * nt;
    a.total = a.carry_den + 2 * nt;
    a.n = n;
    a.ntiles = nt;
    a.beta = fe_host<F>(beta);
    a.gamma = fe_host<F>(gamma);
    a.bd[0] = fe_mul<F>(a.beta, fe_words<F>(h.k1_inv));
    a.bd[1] = a.beta;
    a.bd[2] = fe_mul<F>(a.beta, fe_words<F>(h.k1));
    a.t = Fe<F>::one();
    hipEvent_t pe = c.prof_begin(s);
    hipLaunchKernelGGL((plonk_z_reduce_kernel<F>), dim3((uint32_t)nt), dim3(PLONK_THREADS), 0, s, a);
    c.prof_end("plonk_z_reduce_kernel", pe, s);
    pe = c.prof_begin(s);
    hipLaunchKernelGGL((plonk_z_carry_kernel<F>), dim3(1), dim3(PLONK_TOP), 0, s, a);
    c.prof_end("plonk_z_carry_kernel", pe, s);
    LW_HIP_CHECK(hipGetLastError(), LW_ERR_LAUNCH);
    alignas(16) uint64_t total[4];
    LW_HIP_CHECK(hipMemcpyAsync(total, a.total, 32, hipMemcpyDeviceToHost, s), LW_ERR_LAUNCH);
    LW_HIP_CHECK(hipStreamSynchronize(s), LW_ERR_LAUNCH);
    const Fe<F> den = fe_load<F>(total);
    if (den.is_zero()) {   // the reference's num / den fails on this row (prover.rs:364)
        set_error("round 2: a permutation denominator is zero in rows 0 .. n-2");
        return LW_ERR_INV_ZERO;
    }
    a.t = fe_inv<F>(den);
    pe = c.prof_begin(s);
    hipLaunchKernelGGL((plonk_z_rescan_kernel<F>), dim3((uint32_t)nt), dim3(PLONK_THREADS), 0, s, a);
    c.prof_end("plonk_z_rescan_kernel", pe, s);
    LW_HIP_CHECK(hipGetLastError(), LW_ERR_LAUNCH);
    int rc = ntt_device_locked(c, h.field, LW_LAYOUT_U64_LIMBS_MS_FIRST, LW_DIR_INVERSE, a.z, coef, h.log2n, 1, 0, nullptr, s);
    if (rc) return rc;
    return blind_launch<F>(c, coef, d_out, n, 1, 3, blinders, s);
}

// round 3 on device buffers: d_abc 3 x (n + 2), d_z n + 3, d_out 3 x (n + 3); nothing is waited for
template <class F>
static int round3_locked(Context &c, const lw_plonk_circuit &h, const void *d_abc, const void *d_z, const void *public_input, size_t n_pub,
                         const void *beta, const void *gamma, const void *alpha, const void *blinders, void *d_out, hipStream_t s) {
    const size_t n = h.n, n4 = 4 * n;
    const uint32_t nb = n_pub ? 5 : 4;
    // [stage: the low n coefficients of a b c z, and pi | their extensions to the coset, 4n each]
    if (c.pipe_tmp.ensure((5 * n + 5 * n4) * 32)) return LW_ERR_ALLOC;
    char *stage = (char *)c.pipe_tmp.p, *lde = stage + 5 * n * 32;
    LW_HIP_CHECK(hipMemcpy2DAsync(stage, n * 32, d_abc, (n + 2) * 32, n * 32, 3, hipMemcpyDeviceToDevice, s), LW_ERR_LAUNCH);
    LW_HIP_CHECK(hipMemcpyAsync(stage + 3 * n * 32, d_z, n * 32, hipMemcpyDeviceToDevice, s), LW_ERR_LAUNCH);
    int rc;
    if (n_pub) {   // p_pi = interpolate_fft(public input, zero padded to n)
        char *pi = stage + 4 * n * 32;
        LW_HIP_CHECK(hipMemsetAsync(pi, 0, n * 32, s), LW_ERR_LAUNCH);
        LW_HIP_CHECK(hipMemcpyAsync(pi, public_input, n_pub * 32, hipMemcpyHostToDevice, s), LW_ERR_LAUNCH);
        rc = ntt_device_locked(c, h.field, LW_LAYOUT_U64_LIMBS_MS_FIRST, LW_DIR_INVERSE, pi, pi, h.log2n, 1, 0, nullptr, s);
        if (rc) return rc;
    }
    rc = ntt_device_locked(c, h.field, LW_LAYOUT_U64_LIMBS_MS_FIRST, LW_DIR_FORWARD, stage, lde, h.log2n + 2, nb, 0, h.k1_ref, s, h.log2n);
    if (rc) return rc;
    PlonkQArgs<F> q;
    q.lde = (uint4 *)lde;
    q.cir = (const uint4 *)h.cols.p;
    q.x = (const uint4 *)h.x.p;
    q.p_abc = (const uint4 *)d_abc;
    q.p_z = (const uint4 *)d_z;
    q.n = n;
    q.has_pi = n_pub ? 1 : 0;
    q.beta = fe_host<F>(beta);
    q.gamma = fe_host<F>(gamma);
    q.alpha = fe_host<F>(alpha);
    q.beta_k1 = fe_mul<F>(q.beta, fe_words<F>(h.k1));
    q.beta_k2 = fe_mul<F>(q.beta_k1, fe_words<F>(h.k1));
    q.omega = fe_words<F>(h.omega);
    for (int j = 0; j < 4; j++) {
        q.xn[j] = fe_words<F>(h.xn[j]);
        q.zh_inv[j] = fe_words<F>(h.zh_inv[j]);
    }
    hipEvent_t pe = c.prof_begin(s);
    hipLaunchKernelGGL((plonk_quotient_kernel<F>), dim3((uint32_t)((n4 + PLONK_THREADS - 1) / PLONK_THREADS)), dim3(PLONK_THREADS), 0, s, q);
    c.prof_end("plonk_quotient_kernel", pe, s);
    LW_HIP_CHECK(hipGetLastError(), LW_ERR_LAUNCH);
    // t = interpolate_offset_fft(quotient evaluations, k1): from column a into column b, which has been consumed
    char *t = lde + n4 * 32;
    rc = ntt_device_locked(c, h.field, LW_LAYOUT_U64_LIMBS_MS_FIRST, LW_DIR_INVERSE, lde, t, h.log2n + 2, 1, 0, h.k1_ref, s);
    if (rc) return rc;
    PlonkSplitArgs<F> sp;
    sp.t = (const uint4 *)t;
    sp.out = (uint4 *)d_out;
    sp.n = n;
    sp.b[0] = fe_opt<F>(blinders, 0);
    sp.b[1] = fe_opt<F>(blinders, 1);
    pe = c.prof_begin(s);
    hipLaunchKernelGGL((plonk_t_split_kernel<F>), dim3((uint32_t)((n + 3 + PLONK_THREADS - 1) / PLONK_THREADS), 3), dim3(PLONK_THREADS), 0, s, sp);
    c.prof_end("plonk_t_split_kernel", pe, s);
    LW_HIP_CHECK(hipGetLastError(), LW_ERR_LAUNCH);
    return LW_OK;
}

// host -> the lane's staging on s
static int upload(void *d, const void *h, size_t bytes, hipStream_t s) {
    LW_HIP_CHECK(hipMemcpyAsync(d, h, bytes, hipMemcpyHostToDevice, s), LW_ERR_LAUNCH);
    return LW_OK;
}
static int download_sync(void *h, const void *d, size_t bytes, hipStream_t s) {
    LW_HIP_CHECK(hipMemcpyAsync(h, d, bytes, hipMemcpyDeviceToHost, s), LW_ERR_LAUNCH);
    LW_HIP_CHECK(hipStreamSynchronize(s), LW_ERR_LAUNCH);
    return LW_OK;
}

}  // namespace lw

using namespace lw;

extern "C" {

int lw_plonk_circuit_create(lw_field_t field, size_t n, const void *k1, const void *q_coeffs, const void *s_coeffs, const void *s_lagrange,
                            lw_plonk_circuit_t **out) {
    if (!plonk_field_ok(field)) return LW_ERR_BAD_ARG;
    if (!k1 || !q_coeffs || !s_coeffs || !s_lagrange || !out) return null_arg();
    if (n == 0 || (n & (n - 1))) {
        set_error("Input length is %zu, which is not a power of two", n);
        return LW_ERR_INPUT_NOT_POW2;
    }
    uint32_t lg = 0;
    while (((size_t)1 << lg) < n) lg++;
    if (lg + 2 > field_two_adicity(field)) {
        set_error("no primitive 2^%u-th root of unity in this field", lg + 2);
        return LW_ERR_ROOT_OF_UNITY;
    }
    if (lg + 2 > 34) {
        set_error("2^%u elements exceed device memory", lg + 2);
        return LW_ERR_ALLOC;
    }
    lw_plonk_circuit *h = new (std::nothrow) lw_plonk_circuit{};
    if (!h) return LW_ERR_ALLOC;
    h->field = field;
    h->n = n;
    h->log2n = lg;
    int rc = field == LW_FIELD_STARK252 ? circuit_constants<Stark252>(*h, k1) : circuit_constants<Fr381>(*h, k1);
    if (rc == LW_OK) {
        Entry en(nullptr);
        rc = en.rc;
        hipStream_t s = rc ? nullptr : en.use_lane_stream();
        if (rc == LW_OK && !s) rc = en.rc;
        if (rc == LW_OK) rc = circuit_build(en.c, *h, q_coeffs, s_coeffs, s_lagrange, s);
        if (rc && en.rc == LW_OK) {
            h->s_lagrange.release();
            h->cols.release();
            h->x.release();
        }
    }
    if (rc) {
        delete h;
        return rc;
    }
    *out = h;
    return LW_OK;
}

int lw_plonk_circuit_destroy(lw_plonk_circuit_t *circuit) {
    if (!circuit) return LW_OK;
    Entry en(nullptr);   // binds the context's device for the hipFree
    circuit->s_lagrange.release();
    circuit->cols.release();
    circuit->x.release();
    delete circuit;
    return LW_OK;
}

#define LW_PLONK_DISPATCH(h, fn, ...) ((h)->field == LW_FIELD_STARK252 ? fn<Stark252>(__VA_ARGS__) : fn<Fr381>(__VA_ARGS__))

static int round1_entry(const lw_plonk_circuit_t *h, const void *witness, const void *blinders, void *out, void *hip_stream, bool device) {
    if (!h || !witness || !out) return null_arg();
    if (device && (!aligned16(witness) || !aligned16(out))) return misaligned();
    Entry en(hip_stream);
    if (en.rc) return en.rc;
    Context &c = en.c;
    if (device) return LW_PLONK_DISPATCH(h, round1_locked, c, *h, witness, blinders, out, en.stream);
    hipStream_t s = en.use_lane_stream();
    if (!s) return en.rc;
    const size_t n = h->n;
    if (c.host_io_a.ensure(3 * n * 32) || c.host_io_b.ensure(3 * (n + 2) * 32)) return LW_ERR_ALLOC;
    int rc = upload(c.host_io_a.p, witness, 3 * n * 32, s);
    if (rc == LW_OK) rc = LW_PLONK_DISPATCH(h, round1_locked, c, *h, c.host_io_a.p, blinders, c.host_io_b.p, s);
    if (rc) return rc;
    return download_sync(out, c.host_io_b.p, 3 * (n + 2) * 32, s);
}
int lw_plonk_round1(const lw_plonk_circuit_t *circuit, const void *witness, const void *blinders_or_null, void *out_p_abc) {
    return round1_entry(circuit, witness, blinders_or_null, out_p_abc, nullptr, false);
}
int lw_plonk_round1_device(const lw_plonk_circuit_t *circuit, const void *d_witness, const void *blinders_or_null, void *d_out_p_abc,
                           void *hip_stream) {
    return round1_entry(circuit, d_witness, blinders_or_null, d_out_p_abc, hip_stream, true);
}

static int round2_entry(const lw_plonk_circuit_t *h, const void *witness, const void *beta, const void *gamma, const void *blinders,
                        void *out_z, void *out_p_z, void *hip_stream, bool device) {
    if (!h || !witness || !beta || !gamma || !out_p_z) return null_arg();
    if (device && (!aligned16(witness) || !aligned16(out_z) || !aligned16(out_p_z))) return misaligned();
    Entry en(hip_stream);
    if (en.rc) return en.rc;
    Context &c = en.c;
    if (device) return LW_PLONK_DISPATCH(h, round2_locked, c, *h, witness, beta, gamma, blinders, out_z, out_p_z, en.stream);
    hipStream_t s = en.use_lane_stream();
    if (!s) return en.rc;
    const size_t n = h->n;
    // staging: [witness 3n] and [p_z n + 3 | z n]
    if (c.host_io_a.ensure(3 * n * 32) || c.host_io_b.ensure((2 * n + 3) * 32)) return LW_ERR_ALLOC;
    char *d_pz = (char *)c.host_io_b.p, *d_zv = d_pz + (n + 3) * 32;
    int rc = upload(c.host_io_a.p, witness, 3 * n * 32, s);
    if (rc == LW_OK) rc = LW_PLONK_DISPATCH(h, round2_locked, c, *h, c.host_io_a.p, beta, gamma, blinders, out_z ? d_zv : nullptr, d_pz, s);
    if (rc) return rc;
    if (out_z) LW_HIP_CHECK(hipMemcpyAsync(out_z, d_zv, n * 32, hipMemcpyDeviceToHost, s), LW_ERR_LAUNCH);
    return download_sync(out_p_z, d_pz, (n + 3) * 32, s);
}
int lw_plonk_round2(const lw_plonk_circuit_t *circuit, const void *witness, const void *beta, const void *gamma, const void *blinders_or_null,
                    void *out_z_values_or_null, void *out_p_z) {
    return round2_entry(circuit, witness, beta, gamma, blinders_or_null, out_z_values_or_null, out_p_z, nullptr, false);
}
int lw_plonk_round2_device(const lw_plonk_circuit_t *circuit, const void *d_witness, const void *beta, const void *gamma,
                           const void *blinders_or_null, void *d_out_z_values_or_null, void *d_out_p_z, void *hip_stream) {
    return round2_entry(circuit, d_witness, beta, gamma, blinders_or_null, d_out_z_values_or_null, d_out_p_z, hip_stream, true);
}

static int round3_entry(const lw_plonk_circuit_t *h, const void *p_abc, const void *p_z, const void *public_input, size_t n_pub, const void *beta,
                        const void *gamma, const void *alpha, const void *blinders, void *out_t, void *hip_stream, bool device) {
    if (!h || !p_abc || !p_z || !beta || !gamma || !alpha || !out_t || (n_pub && !public_input)) return null_arg();
    if (n_pub > h->n) {
        set_error("%zu public inputs for %zu gates", n_pub, h->n);
        return LW_ERR_LENGTH_MISMATCH;
    }
    if (device && (!aligned16(p_abc) || !aligned16(p_z) || !aligned16(out_t))) return misaligned();
    Entry en(hip_stream);
    if (en.rc) return en.rc;
    Context &c = en.c;
    if (device) return LW_PLONK_DISPATCH(h, round3_locked, c, *h, p_abc, p_z, public_input, n_pub, beta, gamma, alpha, blinders, out_t, en.stream);
    hipStream_t s = en.use_lane_stream();
    if (!s) return en.rc;
    const size_t n = h->n;
    // staging: [p_abc 3 (n + 2) | p_z n + 3] and [t 3 (n + 3)]
    if (c.host_io_a.ensure((4 * n + 9) * 32) || c.host_io_b.ensure(3 * (n + 3) * 32)) return LW_ERR_ALLOC;
    char *d_abc = (char *)c.host_io_a.p, *d_z = d_abc + 3 * (n + 2) * 32;
    int rc = upload(d_abc, p_abc, 3 * (n + 2) * 32, s);
    if (rc == LW_OK) rc = upload(d_z, p_z, (n + 3) * 32, s);
    if (rc == LW_OK) rc = LW_PLONK_DISPATCH(h, round3_locked, c, *h, d_abc, d_z, public_input, n_pub, beta, gamma, alpha, blinders, c.host_io_b.p, s);
    if (rc) return rc;
    return download_sync(out_t, c.host_io_b.p, 3 * (n + 3) * 32, s);
}
int lw_plonk_round3(const lw_plonk_circuit_t *circuit, const void *p_abc, const void *p_z, const void *public_input, size_t n_pub,
                    const void *beta, const void *gamma, const void *alpha, const void *blinders_or_null, void *out_t) {
    return round3_entry(circuit, p_abc, p_z, public_input, n_pub, beta, gamma, alpha, blinders_or_null, out_t, nullptr, false);
}
int lw_plonk_round3_device(const lw_plonk_circuit_t *circuit, const void *d_p_abc, const void *d_p_z, const void *public_input, size_t n_pub,
                           const void *beta, const void *gamma, const void *alpha, const void *blinders_or_null, void *d_out_t,
                           void *hip_stream) {
    return round3_entry(circuit, d_p_abc, d_p_z, public_input, n_pub, beta, gamma, alpha, blinders_or_null, d_out_t, hip_stream, true);
}

}  // extern "C"
