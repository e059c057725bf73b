"""Stark252 NTTs that drive the fused Montgomery column chains (field.cuh fips_fused, mac_chains.inc FusedCol) through
their edges, bit-exact against the CPU oracle: inputs of all zeros (every column sum and every t_k is 0, so the unit-limb
step runs with no borrow), all p - 1 (the largest canonical limbs), and values whose low u64 limb is 0 (t_0 = t_1 = 0 in
the first products of the first pass); then random inputs at 2^8, 2^16 and 2^20, forward and inverse, plain and coset.
The same columns run on chosen operand pairs, one product per row, in tests/test_gpu_field_pointwise.py."""
import numpy as np
import pytest

from oracle import oracle as O
from tests import util

pytestmark = pytest.mark.gpu

P_LIMBS = [0x0800000000000011, 0, 0, 1]   # p = 2^251 + 17*2^192 + 1, u64 limbs most significant first


def _edge(kind, log_n, seed):
    n = 1 << log_n
    if kind == "zeros":
        return np.zeros((n, 4), np.uint64)
    if kind == "p_minus_1":
        a = np.tile(np.array(P_LIMBS, np.uint64), (n, 1))
        a[:, 3] = 0
        return a
    if kind == "low_limb_0":
        a = util.rand_elems("stark252", n, seed)
        a[:, 3] = 0
        a[-1, 0] |= np.uint64(1)          # non-zero leading coefficient (Polynomial::new strips zeros)
        return a
    if kind == "mixed":                   # alternate p - 1, 0 and low-limb-0 values
        a = util.rand_elems("stark252", n, seed)
        a[:, 3] = 0
        a[0::3] = np.array(P_LIMBS, np.uint64) - np.array([0, 0, 0, 1], np.uint64)
        a[1::3] = 0
        a[-1, 0] |= np.uint64(1)
        return a
    raise ValueError(kind)


def _fld():
    return util.field_pairs()["stark252"]


@pytest.mark.parametrize("kind", ["zeros", "p_minus_1", "low_limb_0", "mixed"])
@pytest.mark.parametrize("log_n", [8, 16])
def test_edge_inputs_forward_inverse(kind, log_n):
    from lambda_elliptic_curves_amd import fft
    fld, oid = _fld()
    a = _edge(kind, log_n, 50 + log_n)
    got = fft.evaluate_fft(fld, a)
    exp = O.evaluate_fft(oid, a)
    assert got.shape == exp.shape and np.array_equal(got, exp)
    inv = fft.interpolate_fft(fld, a)
    assert np.array_equal(inv, O.interpolate_fft(oid, a))


@pytest.mark.parametrize("kind", ["p_minus_1", "low_limb_0"])
@pytest.mark.parametrize("log_n", [8, 16])
def test_edge_inputs_coset(kind, log_n):
    from lambda_elliptic_curves_amd import fft
    fld, oid = _fld()
    a = _edge(kind, log_n, 60 + log_n)
    off = util.offset_elem("stark252", 3)
    ev = fft.evaluate_offset_fft(fld, a, 1, None, off)
    assert np.array_equal(ev, O.evaluate_fft(oid, a, 1, None, off))
    back = fft.interpolate_offset_fft(fld, a, off)
    assert np.array_equal(back, O.interpolate_fft(oid, a, off))


@pytest.mark.parametrize("log_n", [8, 16, 20])
def test_random_forward_inverse_coset(log_n):
    from lambda_elliptic_curves_amd import fft
    fld, oid = _fld()
    a = util.rand_elems("stark252", 1 << log_n, 70 + log_n)
    a[-1, -1] |= np.uint64(1)
    ev = fft.evaluate_fft(fld, a)
    assert np.array_equal(ev, O.evaluate_fft(oid, a))
    co = fft.interpolate_fft(fld, a)
    assert np.array_equal(co, O.interpolate_fft(oid, a))
    off = util.offset_elem("stark252", 7)
    evo = fft.evaluate_offset_fft(fld, a, 1, None, off)
    assert np.array_equal(evo, O.evaluate_fft(oid, a, 1, None, off))
    back = fft.interpolate_offset_fft(fld, evo, off)
    assert np.array_equal(back, O.interpolate_fft(oid, evo, off))
    assert np.array_equal(back, a)
