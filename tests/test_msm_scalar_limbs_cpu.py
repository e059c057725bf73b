"""Scalars of 1 to 8 u64 limbs (lw_hip_msm_limbs, msm(..., scalar_limbs=L)): the host-side checks that need no device,
and the Python mirror's reshaping.  The reference's Pippenger is generic over the width, msm<const NUM_LIMBS, G>
(math/src/msm/pippenger.rs:18-32)."""
import ctypes as C

import numpy as np
import pytest

from lambda_elliptic_curves_amd import _lib, errors, msm

NEW = ("lw_hip_msm_limbs", "lw_hip_msm_limbs_device")


def _vp(a):
    return a.ctypes.data_as(C.c_void_p)


def test_limb_entry_points_are_exported_and_bound():
    L = _lib.lib()
    for sym in NEW:
        assert sym in _lib.EXPORTS
        f = getattr(L, sym)
        assert f.restype is C.c_int
        assert f.argtypes is not None and f.argtypes[2] is C.c_uint32   # scalar_limbs


@pytest.mark.parametrize("limbs", [0, 9, 64])
def test_width_outside_one_to_eight_is_bad_arg_before_any_device_work(limbs):
    L = _lib.lib()
    s = np.ones((2, 8), np.uint64)
    p = np.ones((2, 18), np.uint64)
    out = np.zeros(18, np.uint64)
    assert L.lw_hip_msm_limbs(_lib.CURVE_BLS12_381_G1, _vp(s), limbs, 2, _vp(p), 2, _vp(out)) == _lib.ERR_BAD_ARG
    # the device form refuses the width before it looks at the (here host) pointers or the stream
    assert L.lw_hip_msm_limbs_device(_lib.CURVE_BLS12_381_G1, _vp(s), limbs, _vp(p), 2, _vp(out), None) == _lib.ERR_BAD_ARG
    with pytest.raises(errors.HipError):
        msm.msm(msm.BLS12381Curve, np.ones((2, max(limbs, 1)), np.uint64), p, scalar_limbs=limbs)


def test_length_mismatch_is_checked_first():
    L = _lib.lib()
    s = np.ones((2, 6), np.uint64)
    p = np.ones((3, 18), np.uint64)
    out = np.zeros(18, np.uint64)
    assert L.lw_hip_msm_limbs(_lib.CURVE_BLS12_381_G1, _vp(s), 6, 2, _vp(p), 3, _vp(out)) == _lib.ERR_LENGTH_MISMATCH
    assert L.lw_hip_msm_limbs(_lib.CURVE_BLS12_381_G1, _vp(s), 9, 2, _vp(p), 3, _vp(out)) == _lib.ERR_LENGTH_MISMATCH
    for limbs in (1, 2, 3, 5, 6, 8):
        with pytest.raises(errors.LengthMismatch):
            msm.msm(msm.BLS12381Curve, np.ones((2, limbs), np.uint64), p, scalar_limbs=limbs)
        with pytest.raises(errors.LengthMismatch):
            msm.msm_with(msm.BLS12381Curve, np.ones((2, limbs), np.uint64), p, 4, scalar_limbs=limbs)


def test_other_widths_have_no_cpu_fallback():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    for limbs in (1, 2, 3, 5, 6, 7, 8):
        with pytest.raises(errors.HipError):
            msm.msm(msm.BLS12381Curve, np.ones((3, limbs), np.uint64), np.ones((3, 18), np.uint64), scalar_limbs=limbs)


class _Recorder:
    """stands in for the library: records which MSM entry point was called with what"""

    def __init__(self):
        self.calls = []

    def lw_hip_msm(self, curve, s, n_s, p, n_p, out):
        self.calls.append(("lw_hip_msm", 4, n_s, n_p, np.ctypeslib.as_array(C.cast(s, C.POINTER(C.c_uint64)), (n_s * 4,)).copy()))
        return 0

    def lw_hip_msm_limbs(self, curve, s, limbs, n_s, p, n_p, out):
        self.calls.append(("lw_hip_msm_limbs", limbs, n_s, n_p,
                           np.ctypeslib.as_array(C.cast(s, C.POINTER(C.c_uint64)), (n_s * limbs,)).copy()))
        return 0


def test_msm_reshapes_rows_of_the_given_width(monkeypatch):
    rec = _Recorder()
    monkeypatch.setattr(msm.L, "lib", lambda: rec)
    pts = np.zeros((2, 18), np.uint64)
    cs = np.arange(12, dtype=np.uint64).reshape(2, 6)   # two 6-limb rows = three 4-limb rows
    msm.msm(msm.BLS12381Curve, cs, pts, scalar_limbs=6)
    name, limbs, n_s, n_p, words = rec.calls[-1]
    assert (name, limbs, n_s, n_p) == ("lw_hip_msm_limbs", 6, 2, 2)
    assert np.array_equal(words, cs.reshape(-1))
    # a flat buffer is cut into rows of the given width too
    msm.msm(msm.BLS12381Curve, cs.reshape(-1), pts, scalar_limbs=6)
    assert rec.calls[-1][:4] == ("lw_hip_msm_limbs", 6, 2, 2)
    msm.msm_with(msm.BLS12381Curve, cs, pts, 3, scalar_limbs=6)
    assert rec.calls[-1][:4] == ("lw_hip_msm_limbs", 6, 2, 2)
    # read as 4-limb rows the same words are three scalars for two points
    with pytest.raises(errors.LengthMismatch):
        msm.msm_with(msm.BLS12381Curve, cs, pts, 3)
    # the default width keeps the existing entry point
    msm.msm(msm.BLS12381Curve, np.arange(8, dtype=np.uint64).reshape(2, 4), pts)
    assert rec.calls[-1][:4] == ("lw_hip_msm", 4, 2, 2)
    msm.msm(msm.BLS12381Curve, np.arange(2, dtype=np.uint64).reshape(2, 1), pts, scalar_limbs=1)
    assert rec.calls[-1][:4] == ("lw_hip_msm_limbs", 1, 2, 2)
