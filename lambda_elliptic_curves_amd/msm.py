"""Host-side mirror of math/src/msm/pippenger.rs `msm` for the HIP backend."""
import ctypes as C

import numpy as np

from . import _lib as L
from .errors import check


class Curve:
    def __init__(self, name, curve, coord_words):
        self.name, self.curve, self.coord_words = name, curve, coord_words
        self.point_words = 3 * coord_words

    def __repr__(self):
        return f"Curve({self.name})"


BLS12381Curve = Curve("BLS12381Curve", L.CURVE_BLS12_381_G1, 6)
BN254Curve = Curve("BN254Curve", L.CURVE_BN254_G1, 4)
BN254TwistCurve = Curve("BN254TwistCurve", L.CURVE_BN254_G2, 8)
BLS12381TwistCurve = Curve("BLS12381TwistCurve", L.CURVE_BLS12_381_G2, 12)


def msm_fr(curve, fr_elements, points):
    """msm over FrElements as stored (Montgomery form): representative() + msm in one device call."""
    s = np.ascontiguousarray(fr_elements, dtype=np.uint64).reshape(-1, 4)
    p = np.ascontiguousarray(points, dtype=np.uint64).reshape(-1, curve.point_words)
    out = np.zeros(curve.point_words, dtype=np.uint64)
    check(L.lib().lw_hip_msm_fr(curve.curve, s.ctypes.data_as(C.c_void_p), s.shape[0], p.ctypes.data_as(C.c_void_p),
                                p.shape[0], out.ctypes.data_as(C.c_void_p)))
    return out


def _scalar_rows(cs, scalar_limbs):
    s = np.ascontiguousarray(cs, dtype=np.uint64)
    if 1 <= scalar_limbs <= 8:
        return s.reshape(-1, scalar_limbs)
    return s.reshape(s.shape[0] if s.ndim > 1 else 1, -1)   # a width the library refuses (LW_ERR_BAD_ARG): rows as given


def msm(curve, cs, points, scalar_limbs=4):
    """pippenger::msm(cs, points): cs = (n, scalar_limbs) uint64 canonical scalars (MS limb first), points = (n, 3*coord_words)
    uint64 projective points.  Returns one projective point; only its affine image is canonical.
    Different lengths -> LengthMismatch (pippenger.rs:25-27); empty input -> neutral element.
    scalar_limbs: 1 .. 8, the NUM_LIMBS of the reference's UnsignedInteger<NUM_LIMBS> scalars (pippenger.rs:18-32); the
    sum is over the full integers, not reduced mod r.  4 goes through lw_hip_msm, any other width through lw_hip_msm_limbs."""
    s = _scalar_rows(cs, scalar_limbs)
    p = np.ascontiguousarray(points, dtype=np.uint64).reshape(-1, curve.point_words)
    out = np.zeros(curve.point_words, dtype=np.uint64)
    if scalar_limbs == 4:
        check(L.lib().lw_hip_msm(curve.curve, s.ctypes.data_as(C.c_void_p), s.shape[0], p.ctypes.data_as(C.c_void_p),
                                 p.shape[0], out.ctypes.data_as(C.c_void_p)))
    else:
        check(L.lib().lw_hip_msm_limbs(curve.curve, s.ctypes.data_as(C.c_void_p), scalar_limbs, s.shape[0],
                                       p.ctypes.data_as(C.c_void_p), p.shape[0], out.ctypes.data_as(C.c_void_p)))
    return out


def msm_with(curve, cs, points, window_size, scalar_limbs=4):
    """pippenger::msm_with (math/src/msm/pippenger.rs:42-103).  The window only shapes the reference's schedule;
    the group element is the same for every window, so this is msm() (the device picks its own window)."""
    if len(_scalar_rows(cs, scalar_limbs)) != len(np.asarray(points).reshape(-1, curve.point_words)):
        from .errors import LengthMismatch
        raise LengthMismatch("scalars and points have different lengths")
    return msm(curve, cs, points, scalar_limbs=scalar_limbs)


def msm_device(curve, t_scalars, t_points, n, stream=None, scalar_limbs=4):
    """Device-resident MSM on torch tensors; returns the projective result as a numpy array.  t_scalars holds
    n x scalar_limbs u64 (see msm())."""
    import torch
    if stream is None:
        stream = torch.cuda.current_stream().cuda_stream
    out = np.zeros(curve.point_words, dtype=np.uint64)
    if scalar_limbs == 4:
        check(L.lib().lw_hip_msm_device(curve.curve, C.c_void_p(t_scalars.data_ptr()), C.c_void_p(t_points.data_ptr()), n,
                                        out.ctypes.data_as(C.c_void_p), C.c_void_p(stream)))
    else:
        check(L.lib().lw_hip_msm_limbs_device(curve.curve, C.c_void_p(t_scalars.data_ptr()), scalar_limbs,
                                              C.c_void_p(t_points.data_ptr()), n, out.ctypes.data_as(C.c_void_p),
                                              C.c_void_p(stream)))
    return out


def ec_pointwise_device(curve, op, t_a, t_b, n, t_out, model=0, stream=None):
    """The test seam of the group law (lw_hip_ec_pointwise_device): one formula of csrc/ec.cuh per row of device-resident
    torch tensors, raw (X, Y, Z) into t_out.  op: L.EC_OP_*; t_b: None for EC_OP_DBL and EC_OP_TO_AFFINE; model 1: the
    isomorphic model of the curve."""
    import torch
    if stream is None:
        stream = torch.cuda.current_stream().cuda_stream
    check(L.lib().lw_hip_ec_pointwise_device(curve.curve, model, op, C.c_void_p(t_a.data_ptr()),
                                             C.c_void_p(t_b.data_ptr()) if t_b is not None else None, n,
                                             C.c_void_p(t_out.data_ptr()), C.c_void_p(stream)))
    return t_out


class Srs:
    """A fixed point set kept on the device in affine form (lw_hip_srs_*): what the reference's KZG
    `StructuredReferenceString.powers_main_group` (crypto/src/commitments/kzg.rs:159-163) or a Groth16 proving-key
    vector (provers/groth16/src/prover.rs:69-85) is to repeated msm() calls.  `srs.msm(cs)` equals
    msm(cs, points[:len(cs)]) — fewer scalars than points is the KZG call shape; more is LengthMismatch.
    Sets of 2^19 points and more keep 13 window-shifted copies on the device (include/lw_hip.h: 13 x the affine bytes,
    LW_HIP_SRS_FOLD=0 to keep one); results do not depend on it."""

    def __init__(self, curve, points=None, t_points=None, n=None, stream=None):
        self.curve = curve
        self._h = C.c_void_p()
        if t_points is not None:        # device-resident projective points (torch tensor)
            import torch
            if stream is None:
                stream = torch.cuda.current_stream().cuda_stream
            self.n = int(n if n is not None else t_points.shape[0])
            check(L.lib().lw_hip_srs_create_device(curve.curve, C.c_void_p(t_points.data_ptr()), self.n, C.c_void_p(stream),
                                                   C.byref(self._h)))
        else:
            p = np.ascontiguousarray(points, dtype=np.uint64).reshape(-1, curve.point_words)
            self.n = p.shape[0]
            check(L.lib().lw_hip_srs_create(curve.curve, p.ctypes.data_as(C.c_void_p), self.n, C.byref(self._h)))

    def msm(self, cs):
        s = np.ascontiguousarray(cs, dtype=np.uint64).reshape(-1, 4)
        out = np.zeros(self.curve.point_words, dtype=np.uint64)
        check(L.lib().lw_hip_msm_srs(self._h, s.ctypes.data_as(C.c_void_p), s.shape[0], out.ctypes.data_as(C.c_void_p)))
        return out

    def msm_fr(self, fr_elements):
        s = np.ascontiguousarray(fr_elements, dtype=np.uint64).reshape(-1, 4)
        out = np.zeros(self.curve.point_words, dtype=np.uint64)
        check(L.lib().lw_hip_msm_srs_fr(self._h, s.ctypes.data_as(C.c_void_p), s.shape[0], out.ctypes.data_as(C.c_void_p)))
        return out

    def msm_device(self, t_scalars, n, stream=None):
        import torch
        if stream is None:
            stream = torch.cuda.current_stream().cuda_stream
        out = np.zeros(self.curve.point_words, dtype=np.uint64)
        check(L.lib().lw_hip_msm_srs_device(self._h, C.c_void_p(t_scalars.data_ptr()), n, out.ctypes.data_as(C.c_void_p),
                                            C.c_void_p(stream)))
        return out

    def msm_fr_device(self, t_fr_elements, n, stream=None):
        """Scalars as stored FrElements (Montgomery form) already on the device — e.g. the h coefficients
        groth16.calculate_h_coefficients_device leaves in HBM (provers/groth16/src/prover.rs:68-72,97-101)."""
        import torch
        if stream is None:
            stream = torch.cuda.current_stream().cuda_stream
        out = np.zeros(self.curve.point_words, dtype=np.uint64)
        check(L.lib().lw_hip_msm_srs_fr_device(self._h, C.c_void_p(t_fr_elements.data_ptr()), n, out.ctypes.data_as(C.c_void_p),
                                               C.c_void_p(stream)))
        return out

    def close(self):
        if self._h:
            L.lib().lw_hip_srs_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
