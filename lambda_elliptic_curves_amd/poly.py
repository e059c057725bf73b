"""Polynomial::evaluate and Polynomial::ruffini_division_inplace (math/src/polynomial/mod.rs:98-109, 157-164) on the
device, over Stark252 and BLS12-381 Fr.  Elements are (n, 4) uint64 arrays in the reference's memory form (Montgomery,
MS limb first); points and x are host values in every form."""
import ctypes as C

import numpy as np

from . import _lib as L
from .errors import check


def _elems(a):
    return np.ascontiguousarray(a, dtype=np.uint64).reshape(-1, 4)


def _one(x):
    return np.ascontiguousarray(x, dtype=np.uint64).reshape(-1)[:4].copy()


def _stream(stream):
    if stream is None:
        import torch
        stream = torch.cuda.current_stream().cuda_stream
    return C.c_void_p(stream)


def evaluate(field, polys, points):
    """(K, M, 4) table: [k, j] = polys[k](points[j]).  polys: a list of coefficient arrays of any lengths (0 included)."""
    ps = [_elems(p) for p in polys]
    pts = _elems(points) if len(points) else np.zeros((0, 4), np.uint64)
    out = np.zeros((len(ps), pts.shape[0], 4), np.uint64)
    ptrs = (C.c_void_p * max(1, len(ps)))(*[p.ctypes.data for p in ps])
    lens = (C.c_size_t * max(1, len(ps)))(*[p.shape[0] for p in ps])
    check(L.lib().lw_poly_evaluate(field.field, ptrs, lens, len(ps), pts.ctypes.data_as(C.c_void_p), pts.shape[0],
                                   out.ctypes.data_as(C.c_void_p)))
    return out


def evaluate_device(field, t_polys, lens, points, stream=None):
    """evaluate() on device-resident torch tensors; t_polys[k] holds at least lens[k] elements."""
    pts = _elems(points) if len(points) else np.zeros((0, 4), np.uint64)
    out = np.zeros((len(t_polys), pts.shape[0], 4), np.uint64)
    ptrs = (C.c_void_p * max(1, len(t_polys)))(*[t.data_ptr() for t in t_polys])
    ln = (C.c_size_t * max(1, len(t_polys)))(*[int(n) for n in lens])
    check(L.lib().lw_poly_evaluate_device(field.field, ptrs, ln, len(t_polys), pts.ctypes.data_as(C.c_void_p), pts.shape[0],
                                          out.ctypes.data_as(C.c_void_p), _stream(stream)))
    return out


def ruffini_division(field, coeffs, x):
    """-> (quotient (n - 1, 4), remainder p(x) (4,)); n = 0 and n = 1 give an empty quotient."""
    a = _elems(coeffs)
    n = a.shape[0]
    q = np.zeros((max(0, n - 1), 4), np.uint64)
    rem = np.zeros(4, np.uint64)
    xv = _one(x)
    check(L.lib().lw_poly_ruffini_division(field.field, a.ctypes.data_as(C.c_void_p), n, xv.ctypes.data_as(C.c_void_p),
                                           q.ctypes.data_as(C.c_void_p), rem.ctypes.data_as(C.c_void_p)))
    return q, rem


def ruffini_division_device(field, t_coeffs, n, x, t_quotient, stream=None, remainder=True):
    """Quotient of the first n elements of t_coeffs into t_quotient (n - 1 elements, not overlapping t_coeffs); returns
    the remainder, or None without a synchronisation when remainder=False."""
    rem = np.zeros(4, np.uint64)
    xv = _one(x)
    check(L.lib().lw_poly_ruffini_division_device(field.field, C.c_void_p(t_coeffs.data_ptr()), n, xv.ctypes.data_as(C.c_void_p),
                                                  C.c_void_p(t_quotient.data_ptr()),
                                                  rem.ctypes.data_as(C.c_void_p) if remainder else None, _stream(stream)))
    return rem if remainder else None


def batch_inverse(field, elems):
    """FieldElement::inplace_batch_inverse (math/src/field/element.rs:47-65): (n, 4) array of the inverses; a zero element
    raises FieldError."""
    a = _elems(elems)
    out = np.zeros_like(a)
    check(L.lib().lw_field_batch_inverse(field.field, a.ctypes.data_as(C.c_void_p), a.shape[0], out.ctypes.data_as(C.c_void_p)))
    return out


def batch_inverse_device(field, t_in, n, t_out=None, stream=None):
    """batch_inverse() of the first n elements of a device-resident tensor into t_out (None: in place); synchronises
    once.  -> t_out"""
    t_out = t_in if t_out is None else t_out
    check(L.lib().lw_field_batch_inverse_device(field.field, C.c_void_p(t_in.data_ptr()), int(n), C.c_void_p(t_out.data_ptr()),
                                                _stream(stream)))
    return t_out


def batch_inverse_block():
    """Elements one workgroup of the batch inversion owns (lw_field_batch_inverse_block)."""
    return int(L.lib().lw_field_batch_inverse_block())


def _weights(weights, k, m):
    w = np.ascontiguousarray(weights, dtype=np.uint64).reshape(-1, 4)
    if w.shape[0] != k * m:
        from .errors import LengthMismatch
        raise LengthMismatch(f"{w.shape[0]} weights for {k} polynomials and {m} points")
    return w


def deep_composition(field, polys, points, weights):
    """sum_j quot(sum_k weights[k][j] * polys[k], points[j]) with quot = the Ruffini quotient by (X - points[j])
    (compute_deep_composition_poly, provers/stark/src/prover.rs:643-714, over a K x M weight matrix).
    -> (coefficients (n - 1, 4) with n the longest length, stripped length, evals (K, M, 4)); evals[k, j] = polys[k](points[j])
    where the weight is non-zero and 0 elsewhere."""
    ps = [_elems(p) for p in polys]
    pts = _elems(points)
    k, m = len(ps), pts.shape[0]
    w = _weights(weights, k, m)
    n = max((p.shape[0] for p in ps), default=0)
    out = np.zeros((max(0, n - 1), 4), np.uint64)
    evals = np.zeros((k, m, 4), np.uint64)
    ptrs = (C.c_void_p * max(1, k))(*[p.ctypes.data for p in ps])
    lens = (C.c_size_t * max(1, k))(*[p.shape[0] for p in ps])
    ln = C.c_size_t(0)
    check(L.lib().lw_stark_deep_composition(field.field, ptrs, lens, k, pts.ctypes.data_as(C.c_void_p), m,
                                            w.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p), C.byref(ln),
                                            evals.ctypes.data_as(C.c_void_p)))
    return out, ln.value, evals


def deep_composition_device(field, t_polys, lens, points, weights, t_out, stream=None, evals=True):
    """deep_composition() on device-resident torch tensors into t_out (n - 1 elements, overlapping no input).
    evals=True -> (stripped length, evals (K, M, 4)); evals=False -> None, with nothing waited for."""
    pts = _elems(points)
    k, m = len(t_polys), pts.shape[0]
    w = _weights(weights, k, m)
    ptrs = (C.c_void_p * max(1, k))(*[t.data_ptr() for t in t_polys])
    lnv = (C.c_size_t * max(1, k))(*[int(n) for n in lens])
    ev = np.zeros((k, m, 4), np.uint64) if evals else None
    ln = C.c_size_t(0)
    check(L.lib().lw_stark_deep_composition_device(field.field, ptrs, lnv, k, pts.ctypes.data_as(C.c_void_p), m,
                                                   w.ctypes.data_as(C.c_void_p), C.c_void_p(t_out.data_ptr()),
                                                   C.byref(ln) if evals else None,
                                                   ev.ctypes.data_as(C.c_void_p) if evals else None, _stream(stream)))
    return (ln.value, ev) if evals else None
