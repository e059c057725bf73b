"""GPU parity for the full-size-tile NTT passes that hand a tile from one register step to the next through a single
16-byte plane of LDS (csrc/ntt_kernels.cuh, ntt_exchange): bytes against the CPU oracle, every case run three times
with identical output required, since a missing synchronisation in the hand-over shows as a run-to-run difference.

Sizes: 2^11, 2^13, 2^15 = the run-time-shape kernels (one-pass and two-pass small tiles); 2^16 = FX 8, non-last plus
wave-local last; 2^20 = FX 6 (6,6,8); 2^21 = FX 6, 7 and 8.  Fr381 shares the template at the other occupancy.
Everything goes through lw_hip_ntt_device / lw_hip_ntt_lde_device."""
import functools

import numpy as np
import pytest

from oracle import oracle as O
from tests import util

pytestmark = pytest.mark.gpu

RUNS = 3
POISON = -0x0123456789abcdef


@functools.lru_cache(maxsize=None)
def _input(name, log_n):
    a = util.rand_elems(name, 1 << log_n, 9100 + log_n)
    a[-1, -1] |= np.uint64(1)   # leading coefficient non-zero: evaluate_fft keeps the length
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def _expected(name, log_n, inverse, h):
    _, oid = util.field_pairs()[name]
    off = util.offset_elem(name, h) if h else None
    a = _input(name, log_n)
    exp = O.interpolate_fft(oid, a, off) if inverse else O.evaluate_fft(oid, a, 1, None, off)
    exp.setflags(write=False)
    return exp


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).cuda()


def _host(t):
    return t.cpu().numpy().view(np.uint64)


def _run_three(once):
    """once() -> output bytes of one fresh run; all RUNS outputs must be identical.  Returns the first."""
    outs = [once() for _ in range(RUNS)]
    for k in range(1, RUNS):
        assert np.array_equal(outs[0], outs[k]), f"run {k} differs from run 0 on the same input"
    return outs[0]


CASES = [("stark252", n) for n in (11, 13, 15, 16, 20, 21)] + [("fr381", 16), ("fr381", 20)]


@pytest.mark.parametrize("inverse", [False, True], ids=["forward", "inverse"])
@pytest.mark.parametrize("name,log_n", CASES)
def test_transform_matches_oracle_three_runs(name, log_n, inverse):
    import torch
    from lambda_elliptic_curves_amd import fft
    fld, _ = util.field_pairs()[name]
    t_in = _dev(_input(name, log_n))

    def once():
        t_out = torch.full_like(t_in, POISON)
        fft.ntt_device(fld, t_in, t_out, log_n, inverse=inverse)
        torch.cuda.synchronize()
        return _host(t_out)

    assert np.array_equal(_run_three(once), _expected(name, log_n, inverse, 0))


@pytest.mark.parametrize("inverse", [False, True], ids=["forward", "inverse"])
def test_coset_2_16(inverse):
    import torch
    from lambda_elliptic_curves_amd import fft
    fld, _ = util.field_pairs()["stark252"]
    t_in = _dev(_input("stark252", 16))
    off = util.offset_elem("stark252", 7)

    def once():
        t_out = torch.full_like(t_in, POISON)
        fft.ntt_device(fld, t_in, t_out, 16, inverse=inverse, offset=off)
        torch.cuda.synchronize()
        return _host(t_out)

    assert np.array_equal(_run_three(once), _expected("stark252", 16, inverse, 7))


@pytest.mark.parametrize("inverse", [False, True], ids=["forward", "inverse"])
def test_batch_of_three_with_padding_between_2_16(inverse):
    import torch
    from lambda_elliptic_curves_amd import fft
    fld, _ = util.field_pairs()["stark252"]
    n, batch, stride = 1 << 16, 3, (1 << 16) + 24
    a = _input("stark252", 16)
    buf = np.zeros((batch * stride, 4), np.uint64)
    for b in range(batch):   # the same transform three times: one oracle result serves all
        buf[b * stride:b * stride + n] = a
    t_in = _dev(buf)

    def once():
        t_out = torch.full_like(t_in, POISON)
        fft.ntt_device(fld, t_in, t_out, 16, inverse=inverse, batch=batch, batch_stride=stride)
        torch.cuda.synchronize()
        return _host(t_out)

    got = _run_three(once)
    exp = _expected("stark252", 16, inverse, 0)
    for b in range(batch):
        assert np.array_equal(got[b * stride:b * stride + n], exp), b
        assert (got[b * stride + n:(b + 1) * stride].view(np.int64) == POISON).all(), "wrote between the transforms"


@pytest.mark.parametrize("inverse", [False, True], ids=["forward", "inverse"])
def test_input_and_output_aliased_2_16(inverse):
    import torch
    from lambda_elliptic_curves_amd import fft
    fld, _ = util.field_pairs()["stark252"]
    a = _input("stark252", 16)

    def once():
        t = _dev(a)
        fft.ntt_device(fld, t, t, 16, inverse=inverse)
        torch.cuda.synchronize()
        return _host(t)

    assert np.array_equal(_run_three(once), _expected("stark252", 16, inverse, 0))


def test_low_degree_extension_2_13_to_2_16():
    import torch
    from lambda_elliptic_curves_amd import fft
    fld, oid = util.field_pairs()["stark252"]
    a = _input("stark252", 13)
    off = util.offset_elem("stark252", 3)
    t_in = _dev(a)

    def once():
        t_out = torch.full((1 << 16, 4), POISON, dtype=torch.int64, device="cuda")
        fft.lde_device(fld, t_in, 13, t_out, 16, offset=off)
        torch.cuda.synchronize()
        return _host(t_out)

    assert np.array_equal(_run_three(once), O.evaluate_fft(oid, a, 8, 1 << 13, off))
