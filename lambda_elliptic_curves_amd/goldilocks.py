"""NTT over Goldilocks, p = 2^64 - 2^32 + 1, on the HIP backend: Polynomial::evaluate_fft / interpolate_fft and their
offset forms (math/src/fft/polynomial.rs:25-127) for the reference's U64TestField and Winterfell Felt, the low-degree
extension and the pointwise product.

An element is one uint64, the residue itself (no Montgomery form).  Any word is accepted and read mod p; every word of a
result is the canonical residue.  Host arrays are numpy uint64; the device entry points take torch int64 tensors of the
same bytes, resident in HBM, and run on torch's current stream.  `root` is the primitive 2^32-th root of unity the
domain is built from: 0 selects the reference's TWO_ADIC_PRIMITVE_ROOT_OF_UNITY, a field type with another constant
passes its own.
"""
import numpy as np

from . import _lib as L
from .errors import InputError, check

P = (1 << 64) - (1 << 32) + 1
TWO_ADICITY = 32
TWO_ADIC_PRIMITIVE_ROOT_OF_UNITY = 1753635133440165772   # 7^((p - 1) / 2^32)
# RootsConfig (math/src/field/traits.rs)
ROOTS_NATURAL, ROOTS_NATURAL_INVERSED, ROOTS_BIT_REVERSE, ROOTS_BIT_REVERSE_INVERSED = 0, 1, 2, 3


def _words(a):
    return np.ascontiguousarray(a, dtype=np.uint64).reshape(-1)


def _offset_arg(offset):
    return None if offset is None else np.array([int(offset) & ((1 << 64) - 1)], np.uint64)


def ntt(data, inverse=False, log2n=None, batch=1, batch_stride=0, offset=None, root=0, out=None):
    """Backend seam on host buffers: `batch` transforms of 2^log2n words each, `batch_stride` words apart (0: dense).
    The slice is already power-of-two sized.  `out`: write the result into this array instead of a new one."""
    a = _words(data)
    if log2n is None:
        n = a.shape[0] // batch
        if n == 0 or n & (n - 1):
            raise InputError(f"Input length is {n}, which is not a power of two")
        log2n = n.bit_length() - 1
    if out is None:
        out = a.copy() if batch_stride else np.empty_like(a)   # the words between strided columns are the input's
    elif out.nbytes != a.nbytes or out.dtype != a.dtype or not out.flags.c_contiguous:
        raise ValueError("out must be a C-contiguous array of the input's size and type")
    off = _offset_arg(offset)
    check(L.lib().lw_goldilocks_ntt(L.DIR_INVERSE if inverse else L.DIR_FORWARD, L.host_ptr(a), L.host_ptr(out), log2n, batch, batch_stride,
                                    L.host_ptr(off), root))
    return out


def evaluate_fft(coeffs, blowup_factor=1, domain_size=None, offset=None, root=0):
    """Polynomial::evaluate_fft (offset=None) / evaluate_offset_fft (fft/polynomial.rs:25-38): trailing zero coefficients
    are stripped, len = max(coeff_len, domain_size).next_power_of_two() * blowup_factor, and the zero polynomial gives
    len zeros without a transform."""
    a = _words(coeffs)
    nz = np.flatnonzero((a != 0) & (a != np.uint64(P)))
    n = int(nz[-1]) + 1 if nz.size else 0
    size = max(n, 0 if domain_size is None else int(domain_size))
    length = (1 << max(size - 1, 0).bit_length()) * int(blowup_factor)
    if n == 0:
        return np.zeros(length, np.uint64)
    if length == 0 or length & (length - 1):
        raise InputError(f"Input length is {length}, which is not a power of two")
    padded = np.zeros(length, np.uint64)
    padded[:n] = a[:n]
    return ntt(padded, offset=offset, root=root)


def evaluate_offset_fft(coeffs, blowup_factor, domain_size, offset, root=0):
    return evaluate_fft(coeffs, blowup_factor, domain_size, offset, root)


def interpolate_fft(evals, offset=None, strip=False, root=0):
    """Polynomial::interpolate_fft / interpolate_offset_fft.  Returns all n coefficients; strip=True applies
    Polynomial::new's removal of trailing zero coefficients."""
    a = _words(evals)
    n = a.shape[0]
    if n == 0 or n & (n - 1):
        raise InputError(f"Input length is {n}, which is not a power of two")
    out = ntt(a, inverse=True, offset=offset, root=root)
    if strip:
        nz = np.flatnonzero(out)
        out = out[:int(nz[-1]) + 1 if nz.size else 0]
    return out


def interpolate_offset_fft(evals, offset, root=0):
    return interpolate_fft(evals, offset, root=root)


def get_twiddles(order, config, root=0):
    """roots_of_unity::get_twiddles: 2^order / 2 powers of the primitive 2^order-th root (or its inverse), natural or
    bit-reversed."""
    count = (1 << order) // 2 if 0 <= order <= 30 else 0
    out = np.empty(count, np.uint64)
    check(L.lib().lw_goldilocks_gen_twiddles(order, config, root, L.host_ptr(out)))
    return out


def ntt_device(t_in, t_out, log2n, inverse=False, batch=1, batch_stride=0, offset=None, root=0, stream=None):
    """Device-resident transform of `batch` columns of 2^log2n words, `batch_stride` words apart (0: dense); t_out may be
    t_in.  Asynchronous on `stream` (default: torch's current stream)."""
    off = _offset_arg(offset)
    check(L.lib().lw_goldilocks_ntt_device(L.DIR_INVERSE if inverse else L.DIR_FORWARD, L.device_ptr(t_in),
                                           L.device_ptr(t_out), log2n, batch, batch_stride, L.host_ptr(off), root, L.stream_ptr(stream)))


def lde_device(t_coeffs, log2_coeffs, t_out, log2n, batch=1, in_stride=0, out_stride=0, offset=None, root=0, stream=None):
    """Device-resident low-degree extension: evaluate_offset_fft(poly, blowup, Some(domain), offset) for `batch` blocks
    of 2^log2_coeffs coefficients -> 2^log2n evaluations each, without materialising the zero padding."""
    off = _offset_arg(offset)
    check(L.lib().lw_goldilocks_lde_device(L.device_ptr(t_coeffs), log2_coeffs, in_stride, L.device_ptr(t_out),
                                           log2n, out_stride, batch, L.host_ptr(off), root, L.stream_ptr(stream)))


def mul_device(t_a, t_b, t_out, n=None, stream=None):
    """t_out[i] = t_a[i] * t_b[i] mod p for n words (default: all of t_a); t_out may be t_a or t_b."""
    check(L.lib().lw_goldilocks_mul_device(L.device_ptr(t_a), L.device_ptr(t_b), L.device_ptr(t_out),
                                           t_a.numel() if n is None else n, L.stream_ptr(stream)))
