"""KateZaveruchaGoldberg::open / open_batch (crypto/src/commitments/kzg.rs:171-180, 206-226) against a device-cached SRS
(msm.Srs): the quotient by (X - x) is computed on the device and committed there with the SRS MSM.  Coefficients, x and
upsilon are scalar-field elements as stored (Montgomery form, (n, 4) uint64, MS limb first); the scalar field is the SRS
curve's (BLS12-381 -> Fr381, BN254 -> Fr254).  The reference's y argument is not taken: it changes only coefficient 0,
which no quotient coefficient reads.  Each call returns (proof, value): the projective proof point, and p(x) (open) or
the individual values p_k(x) as a (K, 4) array (open_batch)."""
import ctypes as C

import numpy as np

from . import _lib as L
from .errors import check
from .poly import _elems, _one, _stream


def _ups(upsilon):
    return _one(upsilon) if upsilon is not None else np.zeros(4, np.uint64)


def open(srs, coeffs, x):
    a = _elems(coeffs)
    xv = _one(x)
    proof = np.zeros(srs.curve.point_words, np.uint64)
    ev = np.zeros(4, np.uint64)
    check(L.lib().lw_kzg_open(srs._h, a.ctypes.data_as(C.c_void_p), a.shape[0], xv.ctypes.data_as(C.c_void_p),
                              proof.ctypes.data_as(C.c_void_p), ev.ctypes.data_as(C.c_void_p)))
    return proof, ev


def open_device(srs, t_coeffs, n, x, stream=None):
    xv = _one(x)
    proof = np.zeros(srs.curve.point_words, np.uint64)
    ev = np.zeros(4, np.uint64)
    check(L.lib().lw_kzg_open_device(srs._h, C.c_void_p(t_coeffs.data_ptr()), n, xv.ctypes.data_as(C.c_void_p),
                                     proof.ctypes.data_as(C.c_void_p), ev.ctypes.data_as(C.c_void_p), _stream(stream)))
    return proof, ev


def open_batch(srs, polys, x, upsilon):
    ps = [_elems(p) for p in polys]
    xv, uv = _one(x), _ups(upsilon)
    ptrs = (C.c_void_p * max(1, len(ps)))(*[p.ctypes.data for p in ps])
    lens = (C.c_size_t * max(1, len(ps)))(*[p.shape[0] for p in ps])
    proof = np.zeros(srs.curve.point_words, np.uint64)
    evs = np.zeros((len(ps), 4), np.uint64)
    check(L.lib().lw_kzg_open_batch(srs._h, ptrs, lens, len(ps), xv.ctypes.data_as(C.c_void_p), uv.ctypes.data_as(C.c_void_p),
                                    proof.ctypes.data_as(C.c_void_p), evs.ctypes.data_as(C.c_void_p)))
    return proof, evs


def open_batch_device(srs, t_polys, lens, x, upsilon, stream=None):
    xv, uv = _one(x), _ups(upsilon)
    ptrs = (C.c_void_p * max(1, len(t_polys)))(*[t.data_ptr() for t in t_polys])
    ln = (C.c_size_t * max(1, len(t_polys)))(*[int(n) for n in lens])
    proof = np.zeros(srs.curve.point_words, np.uint64)
    evs = np.zeros((len(t_polys), 4), np.uint64)
    check(L.lib().lw_kzg_open_batch_device(srs._h, ptrs, ln, len(t_polys), xv.ctypes.data_as(C.c_void_p),
                                           uv.ctypes.data_as(C.c_void_p), proof.ctypes.data_as(C.c_void_p),
                                           evs.ctypes.data_as(C.c_void_p), _stream(stream)))
    return proof, evs
