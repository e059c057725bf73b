//! lambdaworks-hip — safe wrappers over liblw_hip.so (include/lw_hip.h): the MI355X (gfx950) NTT + MSM backend.
//!
//! UNVERIFIED: written without a Rust toolchain (see README.md).
//!
//! This crate knows nothing about lambdaworks' types: every function takes raw element slices whose bytes are the
//! reference's in-memory representation (Montgomery form, `u64` limbs most significant first — exactly what
//! `FieldElement::value()` holds, math/src/gpu/cuda/field/element.rs:30-42 passes the same bytes to CUDA).  The typed
//! entry points (`evaluate_fft_hip`, `interpolate_fft_hip`, `msm_hip`) live in the lambdaworks tree
//! (rust-shim/lambdaworks/…), the way the CUDA ones live in math/src/fft/gpu/cuda/polynomial.rs.
pub mod error;
pub mod ffi;

pub use error::{check, HipError};
pub use ffi::{Curve, Dir, Field, Layout};

use core::ffi::{c_int, c_void};
use core::mem::size_of;
use core::ptr;

/// One context per process, bound to one device (`lw_hip_init`).  Optional: every entry point initialises lazily on
/// the calling thread's current device.
pub fn init(device: Option<i32>) -> Result<(), HipError> {
    // SAFETY: the pointer is valid for one c_int or NULL with n = 0.
    let rc = unsafe {
        match device {
            Some(d) => ffi::lw_hip_init(&d as *const c_int, 1),
            None => ffi::lw_hip_init(ptr::null(), 0),
        }
    };
    check(rc)
}

pub fn shutdown() {
    // SAFETY: no arguments; idempotent.
    unsafe { ffi::lw_hip_shutdown() }
}

pub fn device_count() -> usize {
    // SAFETY: no arguments.
    unsafe { ffi::lw_hip_device_count().max(0) as usize }
}

pub fn field_elem_bytes(field: Field, layout: Layout) -> usize {
    // SAFETY: pure function of its arguments.
    unsafe { ffi::lw_hip_field_elem_bytes(field, layout) }
}

pub fn curve_point_bytes(curve: Curve) -> usize {
    // SAFETY: pure function of its arguments.
    unsafe { ffi::lw_hip_curve_point_bytes(curve) }
}

/// Marker for element types that are plain data: any bit pattern of `size_of::<Self>()` bytes is a valid value, there is
/// no padding, no `Drop` and no interior pointer.  The library fills such values byte for byte.
///
/// # Safety
/// Implement it only for types for which that holds — `[u64; N]`, and the `#[repr(transparent)]`-style newtype nesting of
/// `FieldElement<MontgomeryBackendPrimeField<_, N>>` (math/src/field/element.rs:40-42, unsigned_integer/element.rs:29-37),
/// which the typed modules under rust-shim/lambdaworks/ assert by size.
pub unsafe trait Pod: Copy + 'static {}
unsafe impl Pod for u32 {}
unsafe impl Pod for u64 {}
unsafe impl<const N: usize> Pod for [u64; N] {}
unsafe impl<const N: usize> Pod for [u32; N] {}

fn check_elems<T>(field: Field, layout: Layout) -> Result<(), HipError> {
    if size_of::<T>() != field_elem_bytes(field, layout) {
        return Err(HipError::BadArgument(format!(
            "element type is {} bytes, the backend expects {} for {:?}/{:?}",
            size_of::<T>(),
            field_elem_bytes(field, layout),
            field,
            layout
        )));
    }
    Ok(())
}

/// The backend seam on host slices — what `evaluate_fft_cuda` / `interpolate_fft_cuda` are to CUDA
/// (math/src/fft/gpu/cuda/polynomial.rs:16-49).  `input.len()` must be a power of two (it is the already padded
/// coefficient / evaluation vector); `T` is the element type as it sits in memory.  `Dir::Inverse` results are already
/// multiplied by N^-1.  `coset_offset`: one domain-field element (same layout's base word) or `None`.
pub fn ntt<T: Pod, O: Pod>(field: Field, layout: Layout, dir: Dir, input: &[T], coset_offset: Option<&O>) -> Result<Vec<T>, HipError> {
    // SAFETY: T and O are Pod.
    unsafe { ntt_unchecked(field, layout, dir, input, coset_offset) }
}

/// [`ntt`] without the `Pod` bounds, for element types the caller vouches for (the typed lambdaworks modules: a
/// `FieldElement<F>` whose `field_name()` and size matched a kernel family is the bare limb array).
///
/// # Safety
/// `T` must be plain data of exactly the backend's element size: every byte pattern the library writes must be a valid
/// `T`, `T` must not implement `Drop`; `O` likewise must be readable as raw bytes of one domain-field element.
pub unsafe fn ntt_unchecked<T, O>(field: Field, layout: Layout, dir: Dir, input: &[T], coset_offset: Option<&O>) -> Result<Vec<T>, HipError> {
    check_elems::<T>(field, layout)?;
    let n = input.len();
    if n == 0 || !n.is_power_of_two() {
        return Err(HipError::InputNotPowerOfTwo(format!("Input length is {n}, which is not a power of two")));
    }
    let mut out: Vec<T> = Vec::with_capacity(n);
    let off = coset_offset.map_or(ptr::null(), |o| o as *const O as *const c_void);
    // SAFETY: `input` holds n elements of the size the library expects (checked above); `out` has capacity for n; the
    // library writes exactly n elements on success and retains no pointer.  (A fresh Vec has never been touched: the
    // library asks for huge pages on it and populates it while the upload and the kernels run, include/lw_hip.h.)
    let rc = unsafe {
        ffi::lw_hip_ntt(field, layout, dir, input.as_ptr() as *const c_void, out.as_mut_ptr() as *mut c_void, n.trailing_zeros(), 1, 0, off)
    };
    check(rc)?;
    // SAFETY: all n elements were initialised by the call above and T: Pod accepts any bytes.
    unsafe { out.set_len(n) };
    Ok(out)
}

/// The same transform into a caller-provided slice (`out.len() == input.len()`): no allocation, and the place to pass a
/// [`HipBuf`] so that the download lands in pinned memory.
pub fn ntt_into<T: Pod, O: Pod>(field: Field, layout: Layout, dir: Dir, input: &[T], out: &mut [T], coset_offset: Option<&O>) -> Result<(), HipError> {
    check_elems::<T>(field, layout)?;
    let n = input.len();
    if n == 0 || !n.is_power_of_two() {
        return Err(HipError::InputNotPowerOfTwo(format!("Input length is {n}, which is not a power of two")));
    }
    if out.len() != n {
        return Err(HipError::BadArgument(format!("output slice holds {} elements, the transform has {n}", out.len())));
    }
    let off = coset_offset.map_or(ptr::null(), |o| o as *const O as *const c_void);
    // SAFETY: both slices are valid for n elements of the checked size; `in` may alias `out`; nothing is retained.
    let rc = unsafe {
        ffi::lw_hip_ntt(field, layout, dir, input.as_ptr() as *const c_void, out.as_mut_ptr() as *mut c_void, n.trailing_zeros(), 1, 0, off)
    };
    check(rc)
}

/// A result buffer from the library's pool of pinned, resident host memory (`lw_hip_result_acquire`): derefs to `[T]`,
/// goes back to the pool on drop.  Downloads into it run at the PCIe rate; a fresh `Vec` of the same size first pays one
/// page fault per 4 KiB.  For provers that keep evaluation vectors alive across calls (the LDE columns of a STARK round).
pub struct HipBuf<T: Pod> {
    ptr: ptr::NonNull<T>,
    len: usize,
}
impl<T: Pod> HipBuf<T> {
    pub fn new(len: usize) -> Result<Self, HipError> {
        let mut p: *mut c_void = ptr::null_mut();
        // SAFETY: out pointer valid; the library returns memory aligned for any element type (page aligned).
        check(unsafe { ffi::lw_hip_result_acquire(len.max(1) * size_of::<T>(), &mut p) })?;
        // memory from the pool may hold an earlier result: any bytes are a valid T (Pod)
        Ok(HipBuf { ptr: ptr::NonNull::new(p as *mut T).ok_or_else(|| HipError::AllocateMemory("null result buffer".into()))?, len })
    }
}
impl<T: Pod> core::ops::Deref for HipBuf<T> {
    type Target = [T];
    fn deref(&self) -> &[T] {
        // SAFETY: ptr is valid for len elements until drop.
        unsafe { core::slice::from_raw_parts(self.ptr.as_ptr(), self.len) }
    }
}
impl<T: Pod> core::ops::DerefMut for HipBuf<T> {
    fn deref_mut(&mut self) -> &mut [T] {
        // SAFETY: unique owner.
        unsafe { core::slice::from_raw_parts_mut(self.ptr.as_ptr(), self.len) }
    }
}
impl<T: Pod> Drop for HipBuf<T> {
    fn drop(&mut self) {
        // SAFETY: the pointer came from lw_hip_result_acquire and is released exactly once.
        unsafe { ffi::lw_hip_result_release(self.ptr.as_ptr() as *mut c_void) };
    }
}
// SAFETY: plain memory owned by the value.
unsafe impl<T: Pod> Send for HipBuf<T> {}

/// `batch` transforms of 2^log2n elements, `stride` elements apart, in place of a rayon loop over columns
/// (provers/stark/src/trace.rs:186-190): one call, one upload.
pub fn ntt_batch_in_place<T: Pod>(field: Field, layout: Layout, dir: Dir, data: &mut [T], log2n: u32, batch: u32, stride: usize) -> Result<(), HipError> {
    check_elems::<T>(field, layout)?;
    let n = 1usize << log2n;
    let stride_eff = if stride == 0 { n } else { stride };
    if batch as usize > 0 && (batch as usize - 1) * stride_eff + n > data.len() {
        return Err(HipError::BadArgument("batch does not fit the slice".into()));
    }
    // SAFETY: extent checked above; `in` may alias `out` (include/lw_hip.h).
    let rc = unsafe {
        ffi::lw_hip_ntt(field, layout, dir, data.as_ptr() as *const c_void, data.as_mut_ptr() as *mut c_void, log2n, batch, stride, ptr::null())
    };
    check(rc)
}

/// `msm::pippenger::msm` on host slices: `scalars` are canonical U256 integers (4 x u64, most significant limb first —
/// what `.representative()` returns), `points` projective points as they sit in memory (`P` = the point type).
/// Returns the normalised representative (x/z : y/z : 1) or (0 : 1 : 0).
pub fn msm<P: Copy>(curve: Curve, scalars: &[[u64; 4]], points: &[P]) -> Result<P, HipError> {
    if size_of::<P>() != curve_point_bytes(curve) {
        return Err(HipError::BadArgument(format!("point type is {} bytes, the backend expects {}", size_of::<P>(), curve_point_bytes(curve))));
    }
    let mut out = core::mem::MaybeUninit::<P>::uninit();
    // SAFETY: slices are valid for their lengths; the library writes one point of curve_point_bytes(curve) bytes on
    // success (also for empty input: the neutral element) and nothing is retained.
    let rc = unsafe {
        ffi::lw_hip_msm(curve, scalars.as_ptr() as *const u64, scalars.len(), points.as_ptr() as *const c_void, points.len(), out.as_mut_ptr() as *mut c_void)
    };
    check(rc)?;
    // SAFETY: initialised by the successful call.
    Ok(unsafe { out.assume_init() })
}

/// [`msm`] for scalars of `L` limbs, 1 <= L <= 8 — `UnsignedInteger<L>` as it sits in memory, most significant limb first
/// (math/src/msm/pippenger.rs:18-32 is generic over the width).  The sum is over the full integers, not reduced mod r.
/// `L == 4` is exactly [`msm`].
pub fn msm_limbs<P: Copy, const L: usize>(curve: Curve, scalars: &[[u64; L]], points: &[P]) -> Result<P, HipError> {
    if size_of::<P>() != curve_point_bytes(curve) {
        return Err(HipError::BadArgument(format!("point type is {} bytes, the backend expects {}", size_of::<P>(), curve_point_bytes(curve))));
    }
    if !(1..=8).contains(&L) {
        return Err(HipError::BadArgument(format!("scalars of {L} limbs: 1 ..= 8 supported")));
    }
    let mut out = core::mem::MaybeUninit::<P>::uninit();
    // SAFETY: as in `msm`; [u64; L] rows are 8 L bytes with no padding, which is the layout lw_hip_msm_limbs reads.
    let rc = unsafe {
        ffi::lw_hip_msm_limbs(curve, scalars.as_ptr() as *const u64, L as u32, scalars.len(), points.as_ptr() as *const c_void, points.len(),
                              out.as_mut_ptr() as *mut c_void)
    };
    check(rc)?;
    // SAFETY: initialised by the successful call.
    Ok(unsafe { out.assume_init() })
}

/// Same with the scalars given as stored `FrElement`s (Montgomery form): the `.representative()` loop every reference
/// caller runs on the CPU first (provers/groth16/src/prover.rs:69-78) happens on the device.
pub fn msm_fr<P: Copy>(curve: Curve, fr_elements: &[[u64; 4]], points: &[P]) -> Result<P, HipError> {
    if size_of::<P>() != curve_point_bytes(curve) {
        return Err(HipError::BadArgument("point type has the wrong size".into()));
    }
    let mut out = core::mem::MaybeUninit::<P>::uninit();
    // SAFETY: as in `msm`.
    let rc = unsafe {
        ffi::lw_hip_msm_fr(curve, fr_elements.as_ptr() as *const u64, fr_elements.len(), points.as_ptr() as *const c_void, points.len(), out.as_mut_ptr() as *mut c_void)
    };
    check(rc)?;
    // SAFETY: initialised by the successful call.
    Ok(unsafe { out.assume_init() })
}

/// A fixed point set kept on the device in affine form (`lw_hip_srs_*`): KZG's `srs.powers_main_group`
/// (crypto/src/commitments/kzg.rs:159-163) or a Groth16 proving-key vector (provers/groth16/src/prover.rs:69-85).
pub struct Srs {
    handle: *mut ffi::lw_srs_t,
    curve: Curve,
    len: usize,
}

// SAFETY: the handle is only used through the library, which serialises all calls on its context lock.
unsafe impl Send for Srs {}
unsafe impl Sync for Srs {}

impl Srs {
    pub fn new<P: Copy>(curve: Curve, points: &[P]) -> Result<Self, HipError> {
        if size_of::<P>() != curve_point_bytes(curve) {
            return Err(HipError::BadArgument("point type has the wrong size".into()));
        }
        let mut handle: *mut ffi::lw_srs_t = ptr::null_mut();
        // SAFETY: `points` is valid for its length; `handle` receives an owned handle on success.
        let rc = unsafe { ffi::lw_hip_srs_create(curve, points.as_ptr() as *const c_void, points.len(), &mut handle) };
        check(rc)?;
        Ok(Self { handle, curve, len: points.len() })
    }

    pub fn len(&self) -> usize {
        self.len
    }

    pub fn is_empty(&self) -> bool {
        self.len == 0
    }

    /// `msm(scalars, &points[..scalars.len()])` — fewer scalars than points is the KZG call shape.
    pub fn msm<P: Copy>(&self, scalars: &[[u64; 4]]) -> Result<P, HipError> {
        if size_of::<P>() != curve_point_bytes(self.curve) {
            return Err(HipError::BadArgument("point type has the wrong size".into()));
        }
        let mut out = core::mem::MaybeUninit::<P>::uninit();
        // SAFETY: the handle is live until drop; one point is written on success.
        let rc = unsafe { ffi::lw_hip_msm_srs(self.handle, scalars.as_ptr() as *const u64, scalars.len(), out.as_mut_ptr() as *mut c_void) };
        check(rc)?;
        // SAFETY: initialised by the successful call.
        Ok(unsafe { out.assume_init() })
    }

    /// `KateZaveruchaGoldberg::open(x, y, p)` (crypto/src/commitments/kzg.rs:171-180) with `p` as stored
    /// `FieldElement`s (Montgomery form); returns the proof and p(x).  `y` does not enter: it changes only coefficient 0,
    /// which the quotient does not read (include/lw_hip.h).  The SRS curve fixes the scalar field.
    pub fn open<P: Copy>(&self, coeffs: &[[u64; 4]], x: &[u64; 4]) -> Result<(P, [u64; 4]), HipError> {
        if size_of::<P>() != curve_point_bytes(self.curve) {
            return Err(HipError::BadArgument("point type has the wrong size".into()));
        }
        let mut out = core::mem::MaybeUninit::<P>::uninit();
        let mut eval = [0u64; 4];
        // SAFETY: the handle is live until drop; one point and one element are written on success.
        let rc = unsafe {
            ffi::lw_kzg_open(self.handle, coeffs.as_ptr() as *const u64, coeffs.len(), x.as_ptr(), out.as_mut_ptr() as *mut c_void,
                             eval.as_mut_ptr())
        };
        check(rc)?;
        // SAFETY: initialised by the successful call.
        Ok((unsafe { out.assume_init() }, eval))
    }

    /// `KateZaveruchaGoldberg::open_batch(x, ys, polynomials, upsilon)` (kzg.rs:206-226); returns the proof and the
    /// individual values p_k(x) (the `ys` a prover passes in).
    pub fn open_batch<P: Copy>(&self, polys: &[&[[u64; 4]]], x: &[u64; 4], upsilon: &[u64; 4]) -> Result<(P, Vec<[u64; 4]>), HipError> {
        if size_of::<P>() != curve_point_bytes(self.curve) {
            return Err(HipError::BadArgument("point type has the wrong size".into()));
        }
        let ptrs: Vec<*const u64> = polys.iter().map(|p| p.as_ptr() as *const u64).collect();
        let lens: Vec<usize> = polys.iter().map(|p| p.len()).collect();
        let mut evals = vec![[0u64; 4]; polys.len()];
        let mut out = core::mem::MaybeUninit::<P>::uninit();
        // SAFETY: every pointer is valid for its length; the handle is live; k points' worth of values are written.
        let rc = unsafe {
            ffi::lw_kzg_open_batch(self.handle, ptrs.as_ptr(), lens.as_ptr(), polys.len() as u32, x.as_ptr(), upsilon.as_ptr(),
                                   out.as_mut_ptr() as *mut c_void, evals.as_mut_ptr() as *mut u64)
        };
        check(rc)?;
        // SAFETY: initialised by the successful call.
        Ok((unsafe { out.assume_init() }, evals))
    }
}

/// `Polynomial::evaluate` (math/src/polynomial/mod.rs:98-109) of every polynomial at every point:
/// `out[k * points.len() + j] = polys[k](points[j])`.  `field`: Stark252 or BLS12-381 Fr (4 x u64 Montgomery elements).
pub fn poly_evaluate(field: Field, polys: &[&[[u64; 4]]], points: &[[u64; 4]]) -> Result<Vec<[u64; 4]>, HipError> {
    let ptrs: Vec<*const c_void> = polys.iter().map(|p| p.as_ptr() as *const c_void).collect();
    let lens: Vec<usize> = polys.iter().map(|p| p.len()).collect();
    let mut out = vec![[0u64; 4]; polys.len() * points.len()];
    // SAFETY: every pointer is valid for its length; `out` holds k x m elements.
    let rc = unsafe {
        ffi::lw_poly_evaluate(field, ptrs.as_ptr(), lens.as_ptr(), polys.len() as u32, points.as_ptr() as *const c_void,
                              points.len() as u32, out.as_mut_ptr() as *mut c_void)
    };
    check(rc)?;
    Ok(out)
}

/// `Polynomial::ruffini_division_inplace(x)` (mod.rs:157-164): the quotient (n - 1 coefficients) and the remainder
/// p(x) that the reference pops.
pub fn ruffini_division(field: Field, coeffs: &[[u64; 4]], x: &[u64; 4]) -> Result<(Vec<[u64; 4]>, [u64; 4]), HipError> {
    let mut q = vec![[0u64; 4]; coeffs.len().saturating_sub(1)];
    let mut rem = [0u64; 4];
    // SAFETY: `coeffs` is valid for its length, `q` for n - 1 elements, `rem` for one.
    let rc = unsafe {
        ffi::lw_poly_ruffini_division(field, coeffs.as_ptr() as *const c_void, coeffs.len(), x.as_ptr() as *const c_void,
                                      q.as_mut_ptr() as *mut c_void, rem.as_mut_ptr() as *mut c_void)
    };
    check(rc)?;
    Ok((q, rem))
}

/// `compute_deep_composition_poly` (provers/stark/src/prover.rs:643-714) over a weight matrix:
/// `sum_j quot(sum_k weights[k * m + j] * polys[k], points[j])`, `quot` the Ruffini quotient by `(X - points[j])`.
/// Returns the coefficients with trailing zeros stripped (as `Polynomial::new` leaves them) and the `k x m` table of
/// `polys[k](points[j])` (zero where the weight is zero).
pub fn deep_composition(field: Field, polys: &[&[[u64; 4]]], points: &[[u64; 4]], weights: &[[u64; 4]])
                        -> Result<(Vec<[u64; 4]>, Vec<[u64; 4]>), HipError> {
    assert_eq!(weights.len(), polys.len() * points.len(), "weights: one element per (polynomial, point)");
    let ptrs: Vec<*const c_void> = polys.iter().map(|p| p.as_ptr() as *const c_void).collect();
    let lens: Vec<usize> = polys.iter().map(|p| p.len()).collect();
    let n = lens.iter().copied().max().unwrap_or(0);
    let mut out = vec![[0u64; 4]; n.saturating_sub(1)];
    let mut evals = vec![[0u64; 4]; polys.len() * points.len()];
    let mut len = 0usize;
    // SAFETY: every pointer is valid for its length; `out` holds n - 1 elements, `evals` k x m.
    let rc = unsafe {
        ffi::lw_stark_deep_composition(field, ptrs.as_ptr(), lens.as_ptr(), polys.len() as u32, points.as_ptr() as *const c_void,
                                       points.len() as u32, weights.as_ptr() as *const c_void, out.as_mut_ptr() as *mut c_void,
                                       &mut len, evals.as_mut_ptr() as *mut c_void)
    };
    check(rc)?;
    out.truncate(len);
    Ok((out, evals))
}

/// `FieldElement::inplace_batch_inverse` (math/src/field/element.rs:47-65) on the device; a zero element is
/// `FieldError::InvZeroError`.
pub fn batch_inverse(field: Field, elems: &mut [[u64; 4]]) -> Result<(), HipError> {
    let p = elems.as_mut_ptr() as *mut c_void;
    // SAFETY: `elems` is valid for its length; the call may run in place.
    check(unsafe { ffi::lw_field_batch_inverse(field, p as *const c_void, elems.len(), p) })
}

/// log2 of the common length of multilinear tables; the length must be a power of two (the reference pads, the caller does here).
fn multilinear_vars(len: usize) -> Result<u32, HipError> {
    if !len.is_power_of_two() {
        return Err(HipError::BadArgument("a multilinear table has 2^n elements".into()));
    }
    Ok(len.trailing_zeros())
}

/// `DenseMultilinearPolynomial::evaluate` (math/src/polynomial/dense_multilinear_poly.rs:54-80) of every table at one
/// point: tables of `2^n` elements, `point` of `n`, variable 0 on the most significant bit of the index.
pub fn multilinear_evaluate(field: Field, tables: &[&[[u64; 4]]], point: &[[u64; 4]]) -> Result<Vec<[u64; 4]>, HipError> {
    let n = multilinear_vars(tables.first().map_or(1, |t| t.len()))?;
    if tables.iter().any(|t| t.len() != 1usize << n) || point.len() != n as usize {
        return Err(HipError::BadArgument("tables of 2^n elements and a point of n coordinates".into()));
    }
    let ptrs: Vec<*const c_void> = tables.iter().map(|t| t.as_ptr() as *const c_void).collect();
    let mut out = vec![[0u64; 4]; tables.len()];
    // SAFETY: every table is valid for 2^n elements, `point` for n, `out` for one element per table.
    let rc = unsafe {
        ffi::lw_multilinear_evaluate(field, ptrs.as_ptr(), tables.len() as u32, n, point.as_ptr() as *const c_void,
                                     out.as_mut_ptr() as *mut c_void)
    };
    check(rc)?;
    Ok(out)
}

/// `DenseMultilinearPolynomial::fix_variables`: the table with its first `r.len()` variables bound to `r`.
pub fn multilinear_fix_variables(field: Field, table: &[[u64; 4]], r: &[[u64; 4]]) -> Result<Vec<[u64; 4]>, HipError> {
    let n = multilinear_vars(table.len())?;
    if r.len() > n as usize {
        return Err(HipError::BadArgument("more values than variables".into()));
    }
    let mut out = vec![[0u64; 4]; table.len() >> r.len()];
    // SAFETY: `table` is valid for 2^n elements, `r` for t, `out` for 2^(n - t).
    let rc = unsafe {
        ffi::lw_multilinear_fix_variables(field, table.as_ptr() as *const c_void, n, r.as_ptr() as *const c_void, r.len() as u32,
                                          out.as_mut_ptr() as *mut c_void)
    };
    check(rc)?;
    Ok(out)
}

/// The prover's round of a sumcheck over the product of 1, 2 or 3 tables: `g(0) .. g(K)`.  With `r_prev` every table is
/// first bound to it in place (its first half holds the bound table afterwards) and the round runs over the remaining
/// variables.
pub fn sumcheck_round(field: Field, tables: &mut [&mut [[u64; 4]]], r_prev: Option<&[u64; 4]>) -> Result<Vec<[u64; 4]>, HipError> {
    let n = multilinear_vars(tables.first().map_or(1, |t| t.len()))?;
    if tables.iter().any(|t| t.len() != 1usize << n) {
        return Err(HipError::BadArgument("tables of one length".into()));
    }
    let ptrs: Vec<*mut c_void> = tables.iter_mut().map(|t| t.as_mut_ptr() as *mut c_void).collect();
    let mut out = vec![[0u64; 4]; tables.len() + 1];
    // SAFETY: every table is valid and exclusively borrowed for 2^n elements; `out` holds K + 1 elements.
    let rc = unsafe {
        ffi::lw_sumcheck_round(field, ptrs.as_ptr(), tables.len() as u32, n, r_prev.map_or(core::ptr::null(), |r| r.as_ptr() as *const c_void),
                               out.as_mut_ptr() as *mut c_void)
    };
    check(rc)?;
    Ok(out)
}

/// The table of `eq(point, .)`: `out[i] = prod_j eq(point[j], bit_{n-1-j}(i))`, `2^n` elements for a point of `n`
/// coordinates (the `chis` table of `DenseMultilinearPolynomial::evaluate`).
pub fn multilinear_eq_table(field: Field, point: &[[u64; 4]]) -> Result<Vec<[u64; 4]>, HipError> {
    if point.len() > 30 {
        return Err(HipError::BadArgument("at most 30 variables".into()));
    }
    let mut out = vec![[0u64; 4]; 1usize << point.len()];
    // SAFETY: `point` is valid for n elements, `out` for 2^n.
    let rc = unsafe {
        ffi::lw_multilinear_eq_table(field, point.as_ptr() as *const c_void, point.len() as u32, out.as_mut_ptr() as *mut c_void)
    };
    check(rc)?;
    Ok(out)
}

/// One term of a composed sumcheck: `coeff * prod_{m in tables} T_m`; `None` is the coefficient one.  Every table at most
/// once, at most three tables.
pub struct SumcheckTerm<'a> {
    pub coeff: Option<[u64; 4]>,
    pub tables: &'a [u32],
}

/// The prover's round of a sumcheck over `sum_x E(x) * sum_t c_t * prod_{m in S_t} T_m(x)`: `g(0) .. g(D)` with
/// `D` = the most tables in a term, plus one with `eq`.  At most 4 tables, 8 terms.  `one` is the field's Montgomery one,
/// the coefficient of a term that names none.  With `r_prev` every table and `eq` is first bound to it in place, as in
/// `sumcheck_round`.
pub fn sumcheck_terms_round(field: Field, tables: &mut [&mut [[u64; 4]]], eq: Option<&mut [[u64; 4]]>, terms: &[SumcheckTerm],
                            one: &[u64; 4], r_prev: Option<&[u64; 4]>) -> Result<Vec<[u64; 4]>, HipError> {
    let n = multilinear_vars(tables.first().map_or(1, |t| t.len()))?;
    if tables.iter().any(|t| t.len() != 1usize << n) || eq.as_ref().map_or(false, |e| e.len() != 1usize << n) {
        return Err(HipError::BadArgument("tables of one length".into()));
    }
    let mut masks = Vec::with_capacity(terms.len());
    let mut coeffs = Vec::with_capacity(terms.len());
    let mut deg = 0usize;
    for t in terms {
        let mut mask = 0u32;
        for &m in t.tables {
            if m >= 32 || mask & (1 << m) != 0 {
                return Err(HipError::BadArgument("a term names every table at most once".into()));
            }
            mask |= 1 << m;
        }
        masks.push(mask);
        coeffs.push(t.coeff.unwrap_or(*one));
        deg = deg.max(t.tables.len());
    }
    let all_one = terms.iter().all(|t| t.coeff.is_none());
    let ptrs: Vec<*mut c_void> = tables.iter_mut().map(|t| t.as_mut_ptr() as *mut c_void).collect();
    let mut out = vec![[0u64; 4]; deg + 1 + eq.is_some() as usize];
    let eq_ptr = eq.map_or(core::ptr::null_mut(), |e| e.as_mut_ptr() as *mut c_void);
    // SAFETY: every table and `eq` is valid and exclusively borrowed for 2^n elements; `masks` and `coeffs` hold one entry
    // per term; `out` holds D + 1 elements, D as the library computes it from the masks.
    let rc = unsafe {
        ffi::lw_sumcheck_terms_round(field, ptrs.as_ptr(), tables.len() as u32, eq_ptr, masks.as_ptr(),
                                     if all_one { core::ptr::null() } else { coeffs.as_ptr() as *const c_void }, terms.len() as u32, n,
                                     r_prev.map_or(core::ptr::null(), |r| r.as_ptr() as *const c_void), out.as_mut_ptr() as *mut c_void)
    };
    check(rc)?;
    Ok(out)
}

/// The parts of the composition polynomial and their commitment, as `stark_round2` returns them.
pub struct Round2 {
    /// `n_parts` blocks of `block_len` coefficients, zero padded
    pub parts_coeffs: Vec<[u64; 4]>,
    pub block_len: usize,
    /// stripped length of every part
    pub part_lens: Vec<usize>,
    pub root: [u8; 32],
    /// `(N - 1)` nodes, root first
    pub nodes: Vec<[u8; 32]>,
    /// `n_parts` columns of `N` evaluations on the LDE coset
    pub parts_lde: Vec<[u64; 4]>,
}

/// `round_2_compute_composition_polynomial` (provers/stark/src/prover.rs:428-484) over host arrays: `columns` holds the LDE
/// columns (`n_cols x N`, natural order), `transition_evals` the AIR's `compute_transition` values (`transitions.len() x N`).
pub fn stark_round2(field: Field, columns: &[[u64; 4]], log2_trace: u32, log2_blowup: u32, coset_offset: &[u64; 4],
                    boundary: &[ffi::lw_stark_boundary_t], transitions: &[ffi::lw_stark_transition_t],
                    transition_evals: &[[u64; 4]], n_parts: usize) -> Result<Round2, HipError> {
    let n_lde = 1usize << (log2_trace + log2_blowup);
    assert_eq!(columns.len() % n_lde, 0, "columns: N elements each");
    assert_eq!(transition_evals.len(), transitions.len() * n_lde, "transition_evals: N elements per constraint");
    let parts = n_parts.max(1);
    let block_len = ((n_lde + parts - 1) / parts).next_power_of_two();
    let mut out = Round2 { parts_coeffs: vec![[0u64; 4]; parts * block_len], block_len, part_lens: vec![0usize; parts], root: [0u8; 32],
                           nodes: vec![[0u8; 32]; n_lde - 1], parts_lde: vec![[0u64; 4]; parts * n_lde] };
    // SAFETY: every input is valid for its length; the outputs hold P x L, P, 32 bytes, N - 1 nodes and P x N elements.
    let rc = unsafe {
        ffi::lw_stark_round2(field, columns.as_ptr() as *const c_void, (columns.len() / n_lde) as u32, log2_trace, log2_blowup,
                             coset_offset.as_ptr() as *const c_void, boundary.as_ptr(), boundary.len() as u32, transitions.as_ptr(),
                             transitions.len() as u32, transition_evals.as_ptr() as *const c_void, n_parts as u32,
                             out.parts_coeffs.as_mut_ptr() as *mut c_void, out.part_lens.as_mut_ptr(), out.root.as_mut_ptr(),
                             out.nodes.as_mut_ptr() as *mut u8, out.parts_lde.as_mut_ptr() as *mut c_void)
    };
    check(rc)?;
    Ok(out)
}

/// The AIR's `compute_transition` at every LDE row, from the AIR written as a program of `lw_stark_air_op_t` (include/lw_hip.h):
/// `columns` holds the LDE columns back to back, `2^col_log2_len[c]` elements for column `c` (`None`: `N` each; a periodic
/// column has `period * blowup`), `consts` the challenges and literals the program reads.  Returns `n_transitions x N`
/// elements, row `c` = constraint `c`: the `transition_evals` of `stark_round2`.
pub fn stark_transition_evaluations(field: Field, ops: &[ffi::lw_stark_air_op_t], consts: &[[u64; 4]], columns: &[[u64; 4]],
                                    col_log2_len: Option<&[u32]>, n_cols: usize, log2_trace: u32, log2_blowup: u32,
                                    n_transitions: usize) -> Result<Vec<[u64; 4]>, HipError> {
    let n_lde = 1usize << (log2_trace + log2_blowup);
    let want: usize = match col_log2_len {
        Some(l) => {
            assert_eq!(l.len(), n_cols, "col_log2_len: one entry per column");
            l.iter().map(|&x| 1usize.checked_shl(x).unwrap_or(0)).sum()
        }
        None => n_cols * n_lde,
    };
    assert_eq!(columns.len(), want, "columns: the sum of the column lengths");
    let mut out = vec![[0u64; 4]; n_transitions * n_lde];
    // SAFETY: ops, consts and columns are valid for their lengths; `out` holds n_transitions x N elements.
    let rc = unsafe {
        ffi::lw_stark_transition_evaluations(field, ops.as_ptr(), ops.len() as u32, consts.as_ptr() as *const c_void, consts.len() as u32,
                                             columns.as_ptr() as *const c_void, col_log2_len.map_or(core::ptr::null(), |l| l.as_ptr()),
                                             n_cols as u32, log2_trace, log2_blowup, n_transitions as u32, out.as_mut_ptr() as *mut c_void)
    };
    check(rc)?;
    Ok(out)
}

/// `grinding::generate_nonce` (provers/stark/src/grinding.rs:40-53) on the device: the smallest nonce in `[first, last]`
/// whose hash has `grinding_factor` (1 ..= 63) leading zero bits, or `None`.  `u64::MAX` is never a candidate, as in the
/// reference's `0..u64::MAX`: `last = u64::MAX` means `u64::MAX - 1`.
pub fn stark_grinding_nonce(seed: &[u8; 32], grinding_factor: u8, first: u64, last: u64) -> Result<Option<u64>, HipError> {
    let (mut nonce, mut found) = (0u64, 0 as c_int);
    // SAFETY: the seed is 32 bytes; both outputs are valid for one value.
    let rc = unsafe { ffi::lw_stark_grinding_nonce(seed.as_ptr(), grinding_factor as u32, first, last, &mut nonce, &mut found) };
    check(rc)?;
    Ok(if found != 0 { Some(nonce) } else { None })
}

/// `MerkleTree::get_proof_by_pos` (crypto/src/merkle_tree/merkle.rs:58-91) and the committed rows of device-resident trees:
/// every tree is opened at its own `q` leaf positions, `positions[t * q + s]`.  Returns `(values, paths)` packed tree-major,
/// then query: per (t, s) `rows_per_leaf * n_cols` elements (none for a tree without columns) and `log2(leaves)` nodes,
/// bottom first.
///
/// # Safety
/// The device pointers of every tree must be valid for the sizes its fields describe; `stream` is a HIP stream or null.
pub unsafe fn stark_open_trees_device(trees: &[ffi::lw_stark_tree_t], positions: &[u64], q: usize, stream: *mut c_void)
                                      -> Result<(Vec<[u64; 4]>, Vec<[u8; 32]>), HipError> {
    assert_eq!(positions.len(), trees.len() * q, "positions: q per tree");
    let (mut n_val, mut n_path) = (0usize, 0usize);
    for t in trees {
        if !t.d_columns.is_null() {
            n_val += q * (t.rows_per_leaf as usize) * (t.n_cols as usize);
        }
        n_path += q * (t.log2_rows as usize).saturating_sub((t.rows_per_leaf as usize).saturating_sub(1));
    }
    let mut values = vec![[0u64; 4]; n_val];
    let mut paths = vec![[0u8; 32]; n_path];
    let rc = ffi::lw_stark_open_trees_device(trees.as_ptr(), trees.len() as u32, positions.as_ptr(), q as u32,
                                             values.as_mut_ptr() as *mut c_void, paths.as_mut_ptr() as *mut u8, stream);
    check(rc)?;
    Ok((values, paths))
}

/// `PoseidonCairoStark252::hades_permutation` (crypto/src/hash/poseidon/mod.rs:27-41) on a batch of states, in place.
pub fn poseidon_permute(states: &mut [[[u64; 4]; 3]]) -> Result<(), HipError> {
    let p = states.as_mut_ptr() as *mut c_void;
    // SAFETY: `states` is valid for its length; the call may run in place.
    check(unsafe { ffi::lw_poseidon_permute(p as *const c_void, states.len(), p) })
}

/// `PoseidonCairoStark252::hash(x[i], y[i])` (mod.rs:59-64) for every pair.
pub fn poseidon_hash(x: &[[u64; 4]], y: &[[u64; 4]]) -> Result<Vec<[u64; 4]>, HipError> {
    assert_eq!(x.len(), y.len(), "one y per x");
    let mut out = vec![[0u64; 4]; x.len()];
    // SAFETY: all three buffers hold x.len() elements.
    check(unsafe { ffi::lw_poseidon_hash(x.as_ptr() as *const c_void, y.as_ptr() as *const c_void, x.len(), out.as_mut_ptr() as *mut c_void) })?;
    Ok(out)
}

/// `PoseidonCairoStark252::hash_single(x[i])` (mod.rs:66-71) for every element.
pub fn poseidon_hash_single(x: &[[u64; 4]]) -> Result<Vec<[u64; 4]>, HipError> {
    let mut out = vec![[0u64; 4]; x.len()];
    // SAFETY: both buffers hold x.len() elements.
    check(unsafe { ffi::lw_poseidon_hash_single(x.as_ptr() as *const c_void, x.len(), out.as_mut_ptr() as *mut c_void) })?;
    Ok(out)
}

/// `PoseidonCairoStark252::hash_many` (mod.rs:73-96) of every row of a row-major matrix with `row_len` columns
/// (`row_len = 0`: `n_rows` digests of the empty input).
pub fn poseidon_hash_many(rows: &[[u64; 4]], n_rows: usize, row_len: usize) -> Result<Vec<[u64; 4]>, HipError> {
    assert_eq!(rows.len(), n_rows * row_len, "rows: n_rows x row_len elements");
    let mut out = vec![[0u64; 4]; n_rows];
    // SAFETY: `rows` holds n_rows x row_len elements, `out` n_rows.
    check(unsafe { ffi::lw_poseidon_hash_many(rows.as_ptr() as *const c_void, n_rows, row_len, out.as_mut_ptr() as *mut c_void) })?;
    Ok(out)
}

/// `MerkleTree<TreePoseidon<PoseidonCairoStark252>>::build` (`batch = false`, one column) or
/// `MerkleTree<BatchPoseidonTree<PoseidonCairoStark252>>::build` (`batch = true`) over the rows of `columns`, each a
/// natural-order column of the same power-of-two length; row `i` of the tree is natural row `bitrev(i)` when
/// `bit_reverse`.  Returns the reference's `nodes` (root first, leaves last).
pub fn poseidon_commit_columns(columns: &[&[[u64; 4]]], bit_reverse: bool, batch: bool) -> Result<Vec<[u64; 4]>, HipError> {
    let n = columns.first().map_or(0, |c| c.len());
    assert!(n.is_power_of_two() && columns.iter().all(|c| c.len() == n), "columns: one power-of-two length");
    let flat: Vec<[u64; 4]> = columns.iter().flat_map(|c| c.iter().copied()).collect();
    let mut nodes = vec![[0u64; 4]; 2 * n - 1];
    let mut root = [0u64; 4];
    let mode = if batch { ffi::LW_POSEIDON_LEAF_MANY } else { ffi::LW_POSEIDON_LEAF_SINGLE };
    // SAFETY: `flat` holds n_cols x n elements, `nodes` 2n - 1 elements of 32 bytes, `root` 32 bytes.
    check(unsafe {
        ffi::lw_poseidon_commit_columns(flat.as_ptr() as *const c_void, columns.len() as u32, n.trailing_zeros(), bit_reverse as c_int,
                                        mode, root.as_mut_ptr() as *mut u8, nodes.as_mut_ptr() as *mut u8)
    })?;
    Ok(nodes)
}

/// The device-side `CommonPreprocessedInput` of a PLONK circuit (provers/plonk/src/setup.rs, `lw_plonk_circuit_*`) and the
/// prover's rounds 1-3 on it (provers/plonk/src/prover.rs:311-535, without the commitments).  Elements are stored
/// `FieldElement`s (Montgomery form); `field` is Stark252 or BLS12-381 Fr.
pub struct PlonkCircuit {
    handle: *mut ffi::lw_plonk_circuit_t,
    n: usize,
}

// SAFETY: the handle is read-only after creation and only used through the library.
unsafe impl Send for PlonkCircuit {}
unsafe impl Sync for PlonkCircuit {}

impl PlonkCircuit {
    /// `q_coeffs`: ql, qr, qo, qm, qc; `s_coeffs`: s1, s2, s3 (coefficient form, n each, zero padded); `s_lagrange`:
    /// the three permutation columns in evaluation form.
    pub fn new(field: Field, n: usize, k1: &[u64; 4], q_coeffs: &[[u64; 4]], s_coeffs: &[[u64; 4]], s_lagrange: &[[u64; 4]])
               -> Result<Self, HipError> {
        if q_coeffs.len() != 5 * n || s_coeffs.len() != 3 * n || s_lagrange.len() != 3 * n {
            return Err(HipError::BadArgument("q_coeffs, s_coeffs, s_lagrange must hold 5n, 3n, 3n elements".into()));
        }
        let mut handle: *mut ffi::lw_plonk_circuit_t = ptr::null_mut();
        // SAFETY: every slice is valid for the length checked above; `handle` receives an owned handle on success.
        let rc = unsafe {
            ffi::lw_plonk_circuit_create(field, n, k1.as_ptr() as *const c_void, q_coeffs.as_ptr() as *const c_void,
                                         s_coeffs.as_ptr() as *const c_void, s_lagrange.as_ptr() as *const c_void, &mut handle)
        };
        check(rc)?;
        Ok(Self { handle, n })
    }

    fn blinders<const K: usize>(b: Option<&[[u64; 4]; K]>) -> *const c_void {
        b.map_or(ptr::null(), |b| b.as_ptr() as *const c_void)
    }

    /// `round_1`: p_a | p_b | p_c, n + 2 coefficients each.  `witness`: a | b | c, n values each.
    pub fn round1(&self, witness: &[[u64; 4]], blinders: Option<&[[u64; 4]; 6]>) -> Result<Vec<[u64; 4]>, HipError> {
        if witness.len() != 3 * self.n {
            return Err(HipError::BadArgument("witness must hold 3n values".into()));
        }
        let mut out = vec![[0u64; 4]; 3 * (self.n + 2)];
        // SAFETY: the handle is live until drop; `out` holds 3 (n + 2) elements.
        check(unsafe { ffi::lw_plonk_round1(self.handle, witness.as_ptr() as *const c_void, Self::blinders(blinders), out.as_mut_ptr() as *mut c_void) })?;
        Ok(out)
    }

    /// `round_2`: (the n values z_i, p_z with n + 3 coefficients).
    pub fn round2(&self, witness: &[[u64; 4]], beta: &[u64; 4], gamma: &[u64; 4], blinders: Option<&[[u64; 4]; 3]>)
                  -> Result<(Vec<[u64; 4]>, Vec<[u64; 4]>), HipError> {
        if witness.len() != 3 * self.n {
            return Err(HipError::BadArgument("witness must hold 3n values".into()));
        }
        let mut z = vec![[0u64; 4]; self.n];
        let mut p_z = vec![[0u64; 4]; self.n + 3];
        // SAFETY: the handle is live until drop; `z` holds n elements and `p_z` n + 3.
        check(unsafe {
            ffi::lw_plonk_round2(self.handle, witness.as_ptr() as *const c_void, beta.as_ptr() as *const c_void, gamma.as_ptr() as *const c_void,
                                 Self::blinders(blinders), z.as_mut_ptr() as *mut c_void, p_z.as_mut_ptr() as *mut c_void)
        })?;
        Ok((z, p_z))
    }

    /// `round_3`: t_lo | t_mid | t_hi, n + 3 coefficients each, from round 1's and round 2's outputs.
    #[allow(clippy::too_many_arguments)]
    pub fn round3(&self, p_abc: &[[u64; 4]], p_z: &[[u64; 4]], public_input: &[[u64; 4]], beta: &[u64; 4], gamma: &[u64; 4],
                  alpha: &[u64; 4], blinders: Option<&[[u64; 4]; 2]>) -> Result<Vec<[u64; 4]>, HipError> {
        if p_abc.len() != 3 * (self.n + 2) || p_z.len() != self.n + 3 {
            return Err(HipError::BadArgument("p_abc must hold 3 (n + 2) coefficients and p_z n + 3".into()));
        }
        let mut out = vec![[0u64; 4]; 3 * (self.n + 3)];
        // SAFETY: the handle is live until drop; the inputs have the lengths checked above; `out` holds 3 (n + 3) elements.
        check(unsafe {
            ffi::lw_plonk_round3(self.handle, p_abc.as_ptr() as *const c_void, p_z.as_ptr() as *const c_void,
                                 public_input.as_ptr() as *const c_void, public_input.len(), beta.as_ptr() as *const c_void,
                                 gamma.as_ptr() as *const c_void, alpha.as_ptr() as *const c_void, Self::blinders(blinders),
                                 out.as_mut_ptr() as *mut c_void)
        })?;
        Ok(out)
    }
}

impl Drop for PlonkCircuit {
    fn drop(&mut self) {
        // SAFETY: the handle came from lw_plonk_circuit_create and is destroyed exactly once.
        unsafe {
            ffi::lw_plonk_circuit_destroy(self.handle);
        }
    }
}

impl Drop for Srs {
    fn drop(&mut self) {
        // SAFETY: the handle came from lw_hip_srs_create and is destroyed exactly once.
        unsafe {
            ffi::lw_hip_srs_destroy(self.handle);
        }
    }
}

/// The library-owned RCCL communicator (one process per GPU).  Rank 0 calls `Comm::unique_id()` and hands the bytes to
/// the other processes out of band (a file, MPI, a socket — `ncclGetUniqueId`'s contract); then every process calls
/// `Comm::init` (collective).
pub struct Comm {
    pub rank: i32,
    pub nranks: i32,
}

impl Comm {
    pub fn unique_id() -> Result<[u8; ffi::LW_HIP_COMM_ID_BYTES], HipError> {
        let mut id = [0u8; ffi::LW_HIP_COMM_ID_BYTES];
        // SAFETY: the buffer has the length the header names.
        check(unsafe { ffi::lw_hip_comm_unique_id(id.as_mut_ptr()) })?;
        Ok(id)
    }

    pub fn init(unique_id: &[u8; ffi::LW_HIP_COMM_ID_BYTES], rank: i32, nranks: i32) -> Result<Self, HipError> {
        // SAFETY: the id has the length the header names.
        check(unsafe { ffi::lw_hip_comm_init(unique_id.as_ptr(), rank, nranks) })?;
        Ok(Self { rank, nranks })
    }

    /// One transform of 2^log2n_total elements (or `batch` of them) block-distributed over the ranks; `d_in_local` /
    /// `d_out_local` are DEVICE pointers to this rank's `batch * 2^log2n_total / nranks` elements.  Collective.
    ///
    /// # Safety
    /// Both pointers must be device allocations of that extent on this process's device; `hip_stream` a valid
    /// `hipStream_t` or null.
    #[allow(clippy::too_many_arguments)]
    pub unsafe fn ntt_sharded_device(&self, field: Field, layout: Layout, dir: Dir, d_in_local: *const c_void, d_out_local: *mut c_void,
                                     log2n_total: u32, batch: u32, natural_output: bool, hip_stream: *mut c_void) -> Result<(), HipError> {
        check(ffi::lw_hip_ntt_sharded_device(field, layout, dir, d_in_local, d_out_local, log2n_total, batch, natural_output as c_int, hip_stream))
    }

    /// `msm` over points sharded across the ranks; every rank receives the total.
    ///
    /// # Safety
    /// `d_scalars` / `d_points` must be device allocations of `n_local` scalars / points.
    pub unsafe fn msm_sharded_device<P: Copy>(&self, curve: Curve, d_scalars: *const u64, d_points: *const c_void, n_local: usize,
                                              hip_stream: *mut c_void) -> Result<P, HipError> {
        if size_of::<P>() != curve_point_bytes(curve) {
            return Err(HipError::BadArgument("point type has the wrong size".into()));
        }
        let mut out = core::mem::MaybeUninit::<P>::uninit();
        check(ffi::lw_hip_msm_sharded_device(curve, d_scalars, d_points, n_local, out.as_mut_ptr() as *mut c_void, hip_stream))?;
        Ok(out.assume_init())
    }
}

impl Drop for Comm {
    fn drop(&mut self) {
        // SAFETY: no arguments; releases the communicator if one exists.
        unsafe {
            ffi::lw_hip_comm_shutdown();
        }
    }
}

/// `evaluate_cfft` (math/src/circle/polynomial.rs:18-35) over Mersenne31: the values of the polynomial with these
/// coefficients on the standard coset of the same (power-of-two, at least 2) size, as canonical residues.
pub fn circle_evaluate_cfft(coeffs: &[u32]) -> Result<Vec<u32>, HipError> {
    assert!(coeffs.len().is_power_of_two() && coeffs.len() >= 2, "coeffs: a power of two, at least 2");
    let mut out = vec![0u32; coeffs.len()];
    // SAFETY: both buffers hold coeffs.len() words.
    check(unsafe { ffi::lw_circle_evaluate_cfft(coeffs.as_ptr(), out.as_mut_ptr(), coeffs.len().trailing_zeros(), 1, 0) })?;
    Ok(out)
}

/// `interpolate_cfft` (polynomial.rs:42-72); an empty input gives an empty result, as there.
pub fn circle_interpolate_cfft(evals: &[u32]) -> Result<Vec<u32>, HipError> {
    if evals.is_empty() {
        return Ok(Vec::new());
    }
    assert!(evals.len().is_power_of_two() && evals.len() >= 2, "evals: a power of two, at least 2");
    let mut out = vec![0u32; evals.len()];
    // SAFETY: both buffers hold evals.len() words.
    check(unsafe { ffi::lw_circle_interpolate_cfft(evals.as_ptr(), out.as_mut_ptr(), evals.len().trailing_zeros(), 1, 0) })?;
    Ok(out)
}

/// `evaluate_fft` / `evaluate_offset_fft` (math/src/fft/polynomial.rs:25-82) over Goldilocks, p = 2^64 - 2^32 + 1, on a
/// slice that is already a power of two: one u64 per element, the residue itself (`U64TestField`'s memory), canonical
/// residues out.  `two_adic_root`: 0 for the reference's `TWO_ADIC_PRIMITVE_ROOT_OF_UNITY`, or the caller's own primitive
/// 2^32-th root (a Winterfell-style `Felt`).
pub fn evaluate_fft_goldilocks_hip(coeffs: &[u64], offset: Option<u64>, two_adic_root: u64) -> Result<Vec<u64>, HipError> {
    goldilocks_ntt_hip(0, coeffs, offset, two_adic_root)
}

/// `interpolate_fft` / `interpolate_offset_fft` (polynomial.rs:87-127) over Goldilocks; arguments as
/// `evaluate_fft_goldilocks_hip`.  All n coefficients are returned.
pub fn interpolate_fft_goldilocks_hip(evals: &[u64], offset: Option<u64>, two_adic_root: u64) -> Result<Vec<u64>, HipError> {
    goldilocks_ntt_hip(1, evals, offset, two_adic_root)
}

fn goldilocks_ntt_hip(dir: c_int, input: &[u64], offset: Option<u64>, two_adic_root: u64) -> Result<Vec<u64>, HipError> {
    assert!(input.len().is_power_of_two(), "input: a power of two");
    let mut out = vec![0u64; input.len()];
    let off = offset.as_ref().map_or(core::ptr::null(), |h| h as *const u64);
    // SAFETY: both buffers hold input.len() words; `off` is NULL or points at one u64 that outlives the call.
    check(unsafe {
        ffi::lw_goldilocks_ntt(dir, input.as_ptr(), out.as_mut_ptr(), input.len().trailing_zeros(), 1, 0, off, two_adic_root)
    })?;
    Ok(out)
}

/// Security level of `RescuePrimeOptimized` (crypto/src/hash/rescue_prime/parameters.rs `SecurityLevel`).
#[derive(Clone, Copy, Debug, PartialEq, Eq)]
pub enum RpoLevel {
    Sec128,
    Sec160,
}

impl RpoLevel {
    fn code(self) -> c_int {
        match self {
            RpoLevel::Sec128 => ffi::LW_RPO_128,
            RpoLevel::Sec160 => ffi::LW_RPO_160,
        }
    }
    /// words of the state
    pub fn width(self) -> usize {
        match self {
            RpoLevel::Sec128 => 12,
            RpoLevel::Sec160 => 16,
        }
    }
    /// words of a digest: rate / 2
    pub fn digest_len(self) -> usize {
        match self {
            RpoLevel::Sec128 => 4,
            RpoLevel::Sec160 => 5,
        }
    }
}

/// `RescuePrimeOptimized::permutation` (rescue_prime_optimized.rs:192-202) on a batch of states, in place: `states` holds
/// `width()` Goldilocks words per state, the residues themselves.
pub fn rpo_permute_hip(level: RpoLevel, states: &mut [u64]) -> Result<(), HipError> {
    assert!(states.len() % level.width() == 0, "states: a whole number of states");
    let p = states.as_mut_ptr();
    // SAFETY: one buffer of states.len() words, read and written in place.
    check(unsafe { ffi::lw_rpo_permute(level.code(), p as *const u64, states.len() / level.width(), p) })
}

/// `RescuePrimeOptimized::hash` (rescue_prime_optimized.rs:205-230) of every row of a row-major matrix with `row_len`
/// columns: `digest_len()` words per row.
pub fn rpo_hash_hip(level: RpoLevel, rows: &[u64], n_rows: usize, row_len: usize) -> Result<Vec<u64>, HipError> {
    assert!(rows.len() == n_rows * row_len, "rows: n_rows * row_len words");
    let mut out = vec![0u64; n_rows * level.digest_len()];
    // SAFETY: rows holds n_rows * row_len words, out n_rows digests.
    check(unsafe { ffi::lw_rpo_hash(level.code(), rows.as_ptr(), n_rows, row_len, out.as_mut_ptr()) })?;
    Ok(out)
}

/// The Merkle tree over the rows of `columns` (each a power-of-two column of the same length): leaf = `hash` of the row,
/// node = `hash(left || right)`.  Returns the reference's `nodes`, root first, `digest_len()` words each.
pub fn rpo_commit_columns_hip(level: RpoLevel, columns: &[&[u64]], bit_reverse: bool) -> Result<Vec<u64>, HipError> {
    assert!(!columns.is_empty(), "columns: at least one");
    let n = columns[0].len();
    assert!(n.is_power_of_two() && columns.iter().all(|c| c.len() == n), "columns: one power-of-two length");
    let flat: Vec<u64> = columns.iter().flat_map(|c| c.iter().copied()).collect();
    let d = level.digest_len();
    let mut root = vec![0u64; d];
    let mut nodes = vec![0u64; (2 * n - 1) * d];
    // SAFETY: flat holds columns.len() * n words, root one digest, nodes 2 n - 1 digests.
    check(unsafe {
        ffi::lw_rpo_commit_columns(level.code(), flat.as_ptr(), columns.len() as u32, n.trailing_zeros(), bit_reverse as c_int,
                                   root.as_mut_ptr(), nodes.as_mut_ptr())
    })?;
    Ok(nodes)
}

/// `MonolithMersenne31::<WIDTH, NUM_FULL_ROUNDS>::permutation` (crypto/src/hash/monolith/mod.rs:91-102) on a batch of
/// states, in place: `states` holds `width` Mersenne31 words per state, read mod p, canonical on return.
pub fn monolith_permute_hip(width: usize, rounds: usize, states: &mut [u32]) -> Result<(), HipError> {
    assert!(width != 0 && states.len() % width == 0, "states: a whole number of states");
    let p = states.as_mut_ptr();
    // SAFETY: one buffer of states.len() words, read and written in place.
    check(unsafe { ffi::lw_monolith_permute(width as u32, rounds as u32, p as *const u32, states.len() / width, p) })
}

/// The 8-word digest of every row of a row-major matrix with `row_len` columns, over the width-16 permutation: every chunk
/// of up to 8 words overwrites the front of the state.  No padding: only for rows of one fixed length.
pub fn monolith_hash_hip(rounds: usize, rows: &[u32], n_rows: usize, row_len: usize) -> Result<Vec<u32>, HipError> {
    assert!(rows.len() == n_rows * row_len, "rows: n_rows * row_len words");
    let mut out = vec![0u32; n_rows * 8];
    // SAFETY: rows holds n_rows * row_len words, out n_rows digests.
    check(unsafe { ffi::lw_monolith_hash(rounds as u32, rows.as_ptr(), n_rows, row_len, out.as_mut_ptr()) })?;
    Ok(out)
}

/// `permute(left || right)[0..8]` for every pair of 8-word digests.
pub fn monolith_compress_hip(rounds: usize, left: &[u32], right: &[u32]) -> Result<Vec<u32>, HipError> {
    assert!(left.len() % 8 == 0 && left.len() == right.len(), "left, right: the same number of 8-word digests");
    let mut out = vec![0u32; left.len()];
    // SAFETY: the three buffers hold left.len() / 8 digests each.
    check(unsafe { ffi::lw_monolith_compress(rounds as u32, left.as_ptr(), right.as_ptr(), left.len() / 8, out.as_mut_ptr()) })?;
    Ok(out)
}

/// The Merkle tree over the rows of `columns` (each a power-of-two column of the same length): leaf = the hash of the row,
/// node = the compression of its children.  Returns the reference's `nodes`, root first, 8 words each.
pub fn monolith_commit_columns_hip(rounds: usize, columns: &[&[u32]], bit_reverse: bool) -> Result<Vec<u32>, HipError> {
    assert!(!columns.is_empty(), "columns: at least one");
    let n = columns[0].len();
    assert!(n.is_power_of_two() && columns.iter().all(|c| c.len() == n), "columns: one power-of-two length");
    let flat: Vec<u32> = columns.iter().flat_map(|c| c.iter().copied()).collect();
    let mut root = vec![0u32; 8];
    let mut nodes = vec![0u32; (2 * n - 1) * 8];
    // SAFETY: flat holds columns.len() * n words, root one digest, nodes 2 n - 1 digests.
    check(unsafe {
        ffi::lw_monolith_commit_columns(rounds as u32, flat.as_ptr(), columns.len() as u32, n.trailing_zeros(), bit_reverse as c_int,
                                        root.as_mut_ptr(), nodes.as_mut_ptr())
    })?;
    Ok(nodes)
}
