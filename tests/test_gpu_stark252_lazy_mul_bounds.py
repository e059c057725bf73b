"""fe_mul_lazy on the device with the operands its dropped carry adds rest on, through the public NTT entry points,
bit-exact against the CPU oracle.

fe_mul_lazy(a, b) uses a < p (a[7] <= 2^27) to leave out one add-with-carry in columns 7 to 13 and the exact carry-in
bounds of columns 1 and 2 (tests/test_mac_chain_bounds_cpu.py proves both on a model of the emitted columns).  Here the
same extremes reach the real kernels:
  * b: the data.  Inputs of 2^251 - 1 (b[7] = 2^27 - 1, every lower limb 0xffffffff) and p - 1 put dense all-ones limbs
    into every first-stage product, where columns 1 and 2 reach their largest carry-in for the twiddle at hand.
  * a: the last pass of interpolate_offset_fft multiplies natural output i by h^-i * N^-1 with that factor as a.  The
    offset h is chosen so that the factor of output 1 is, limb for limb, a chosen Montgomery-form value: the largest
    canonical value with a[7] = 2^27 (a[6] = 16, a[0..5] = 0xffffffff), p - 1, and 2^251 - 1.  (A twiddle w^k with
    a[7] = 2^27 has probability 2^-55, so the twiddle tables never get there by themselves.)
fe_mul_lazy and fe_mul_lazy_uniform take the same first operands directly, one product per row, in tests/test_gpu_field_pointwise.py."""
import numpy as np
import pytest

from oracle import oracle as O
from tests import util

pytestmark = pytest.mark.gpu

P = (1 << 251) + 17 * (1 << 192) + 1
R = 1 << 256
A_TOP = (1 << 251) + 16 * (1 << 192) + ((1 << 192) - 1)     # a[7] = 2^27 at its bound, a[6] = 16, lower limbs all ones
A_CASES = {"a7_at_bound": A_TOP, "p_minus_1": P - 1, "dense_ones": (1 << 251) - 1}
assert all(a < P for a in A_CASES.values()) and (A_TOP >> 224) == 1 << 27


def _elem(x):
    """integer (Montgomery form, as stored) -> one element, u64 limbs most significant first"""
    return np.array([(x >> (64 * (3 - i))) & ((1 << 64) - 1) for i in range(4)], np.uint64)


def _offset_for_factor(a_mont, log_n):
    """The coset offset h (memory form) for which h^-1 * N^-1 is stored as exactly a_mont."""
    a_val = a_mont * pow(R, -1, P) % P
    h_val = pow(a_val * (1 << log_n) % P, -1, P)
    return _elem(h_val * R % P)


def _data(kind, n, seed):
    if kind == "dense_ones":
        return np.tile(_elem((1 << 251) - 1), (n, 1))
    if kind == "p_minus_1":
        return np.tile(_elem(P - 1), (n, 1))
    if kind == "mixed":
        a = util.rand_elems("stark252", n, seed)
        a[0::3] = _elem((1 << 251) - 1)
        a[1::3] = _elem(P - 1)
        return a
    raise ValueError(kind)


def _fld():
    return util.field_pairs()["stark252"]


def test_offset_construction():
    # h^-1 * N^-1 in Montgomery form is the chosen value (checked with integers; no device involved)
    for a_mont in A_CASES.values():
        for log_n in (1, 8):
            off = _offset_for_factor(a_mont, log_n)
            h_mont = sum(int(v) << (64 * (3 - i)) for i, v in enumerate(off))
            h_val = h_mont * pow(R, -1, P) % P
            assert pow(h_val, -1, P) * pow(1 << log_n, -1, P) % P * R % P == a_mont


@pytest.mark.parametrize("kind", ["dense_ones", "p_minus_1", "mixed"])
@pytest.mark.parametrize("log_n", [1, 2, 4, 8, 12, 16])
def test_dense_ones_data_forward_inverse(kind, log_n):
    from lambda_elliptic_curves_amd import fft
    fld, oid = _fld()
    a = _data(kind, 1 << log_n, 90 + log_n)
    assert np.array_equal(fft.evaluate_fft(fld, a), O.evaluate_fft(oid, a))
    assert np.array_equal(fft.interpolate_fft(fld, a), O.interpolate_fft(oid, a))


@pytest.mark.parametrize("a_case", sorted(A_CASES))
@pytest.mark.parametrize("kind", ["dense_ones", "p_minus_1", "mixed"])
@pytest.mark.parametrize("log_n", [1, 2, 8, 12])
def test_chosen_first_operand_of_the_scaling_product(a_case, kind, log_n):
    from lambda_elliptic_curves_amd import fft
    fld, oid = _fld()
    off = _offset_for_factor(A_CASES[a_case], log_n)
    a = _data(kind, 1 << log_n, 95 + log_n)
    got = fft.interpolate_offset_fft(fld, a, off)
    assert np.array_equal(got, O.interpolate_fft(oid, a, off))
    ev = fft.evaluate_offset_fft(fld, a, 1, None, off)
    assert np.array_equal(ev, O.evaluate_fft(oid, a, 1, None, off))
