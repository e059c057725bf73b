"""Circle FFT over Mersenne31 (math/src/circle/ of the reference: evaluate_cfft, interpolate_cfft, get_twiddles) on the
HIP backend, and the low-degree extension built from them.

An element is one uint32.  Any word is accepted and read as (w & p) + (w >> 31) with p = 2^31 - 1 (so p means 0); every
word of a result is the canonical residue.  Host arrays are numpy, one transform or a batch `(batch, n)`; the device
entry points take torch int32 tensors resident in HBM and run on torch's current stream.
"""
import numpy as np

from . import _lib as L
from .errors import InputError, check

P = (1 << 31) - 1
TWIDDLES_EVALUATION, TWIDDLES_INTERPOLATION = 0, 1   # TwiddlesConfig


def _log2_len(n):
    """The transform sizes are the powers of two from 2 on (the standard coset of size 1 does not exist)."""
    if n < 2 or n & (n - 1):
        raise InputError(f"Input length is {n}, which is not a power of two of at least 2")
    return n.bit_length() - 1


def _host(entry, a):
    a = np.ascontiguousarray(a, dtype=np.uint32)
    if a.ndim not in (1, 2):
        raise ValueError("one transform (n,) or a batch (batch, n)")
    log2n = _log2_len(a.shape[-1])
    out = np.empty_like(a)
    if a.size:
        check(entry(L.host_ptr(a), L.host_ptr(out), log2n, a.shape[0] if a.ndim == 2 else 1, 0))
    return out


def evaluate_cfft(coeffs):
    """evaluate_cfft: the values on the standard coset of the polynomial with these coefficients in the basis
    {1, y, x, xy, 2x^2 - 1, ...}."""
    return _host(L.lib().lw_circle_evaluate_cfft, coeffs)


def interpolate_cfft(evals):
    """interpolate_cfft: the coefficients of the polynomial with these values on the standard coset (n^-1 included).  An
    empty input gives an empty result, as in the reference."""
    evals = np.ascontiguousarray(evals, dtype=np.uint32)
    if evals.size == 0:
        return np.empty(0, np.uint32)
    return _host(L.lib().lw_circle_interpolate_cfft, evals)


def get_twiddles(log2n, config):
    """get_twiddles(Coset::new_standard(log2n), config): the list of layers, lengths 1, 2, .., n/2 for TWIDDLES_EVALUATION
    and n/2, .., 1 (the inverses) for TWIDDLES_INTERPOLATION."""
    flat = np.empty((1 << log2n) - 1 if 1 <= log2n <= 30 else 1, np.uint32)
    check(L.lib().lw_circle_get_twiddles(log2n, config, L.host_ptr(flat)))
    lengths = [1 << i for i in range(log2n)]
    if config == TWIDDLES_INTERPOLATION:
        lengths.reverse()
    return np.split(flat, np.cumsum(lengths)[:-1])


def evaluate_cfft_device(t_in, t_out, log2n, batch=1, batch_stride=0, stream=None):
    """Device-resident evaluate_cfft of `batch` columns of 2^log2n words, `batch_stride` words apart (0: dense);
    t_out may be t_in.  Asynchronous on `stream` (default: torch's current stream)."""
    check(L.lib().lw_circle_evaluate_cfft_device(L.device_ptr(t_in), L.device_ptr(t_out), log2n, batch,
                                                 batch_stride, L.stream_ptr(stream)))


def interpolate_cfft_device(t_in, t_out, log2n, batch=1, batch_stride=0, stream=None):
    """Device-resident interpolate_cfft; arguments as evaluate_cfft_device."""
    check(L.lib().lw_circle_interpolate_cfft_device(L.device_ptr(t_in), L.device_ptr(t_out), log2n, batch,
                                                    batch_stride, L.stream_ptr(stream)))


def lde_device(t_evals, log2_in, t_out, log2_out, batch=1, in_stride=0, out_stride=0, stream=None):
    """Device-resident low-degree extension: evaluate_cfft(zero_pad(interpolate_cfft(evals), 2^log2_out)) for `batch`
    columns, the coefficients staying on the device and the padding never written."""
    check(L.lib().lw_circle_lde_device(L.device_ptr(t_evals), log2_in, in_stride, L.device_ptr(t_out),
                                       log2_out, out_stride, batch, L.stream_ptr(stream)))
