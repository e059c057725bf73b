"""GPU parity for the Stark252 passes that add a multiple of p on load and subtract without 2p in most butterflies
(csrc/ntt_bound_plan.h, ntt_butterflies in csrc/ntt_kernels.cuh): bytes against the CPU oracle.

Inputs sit at the edges of the value range, where a subtraction that went below zero or a sum that reached 2^256 would
show: every element p - 1, a single p - 1 among zeros, 0 and p - 1 alternating, and one seeded random vector.

Sizes: 2^5, 2^9 = run-time-shape kernels (today's butterflies); 2^11 = one full tile, a single last pass; 2^16 = (8, 8),
the non-last 8-stage kernel as a first pass plus the last pass; 2^20 = (6, 6, 8), a middle pass with a lazy input;
2^21 = 6-, 7- and 8-stage kernels; 2^16 in a batch of three.  Forms: forward, inverse, both on a coset, and the
low-degree extension (blow-up 8).  Everything goes through lw_hip_ntt_device / lw_hip_ntt_lde_device."""
import numpy as np
import pytest

from oracle import oracle as O
from tests import util

pytestmark = pytest.mark.gpu

P = 2**251 + 17 * 2**192 + 1
POISON = -0x0123456789abcdef
LDE_LOG_BLOWUP = 3
SIZES = (5, 9, 11, 16, 20, 21)
FORMS = ("forward", "inverse", "coset-forward", "coset-inverse", "lde")
KINDS = ("all-p-1", "one-p-1", "alternating", "random")
_CACHE_UP_TO = 16   # the 2^16 results also serve the batched cases; larger ones are used once and not kept
_inputs, _expecteds = {}, {}


def _elem(v):
    return np.array([(v >> s) & (2**64 - 1) for s in (192, 128, 64, 0)], np.uint64)   # reference layout, MS limb first


def _input(kind, log_n):
    key = (kind, log_n)
    if key not in _inputs:
        n = 1 << log_n
        if kind == "random":
            a = util.rand_elems("stark252", n, 7300 + log_n)
        else:
            a = np.zeros((n, 4), np.uint64)
            rows = {"all-p-1": slice(None), "one-p-1": slice(n // 3, n // 3 + 1), "alternating": slice(1, None, 2)}[kind]
            a[rows] = _elem(P - 1)
        a.setflags(write=False)
        _inputs[key] = a
    return _inputs[key]


def _in_log(form, log_n):
    return log_n - LDE_LOG_BLOWUP if form == "lde" else log_n


def _offset(form):
    return util.offset_elem("stark252", 7) if form in ("coset-forward", "coset-inverse", "lde") else None


def _expected(kind, log_n, form):
    key = (kind, log_n, form)
    if key in _expecteds:
        return _expecteds[key]
    a = _input(kind, _in_log(form, log_n))
    if form in ("inverse", "coset-inverse"):
        exp = O.interpolate_fft(O.F_STARK252, a, _offset(form))
    elif form == "lde":
        exp = O.evaluate_fft(O.F_STARK252, a, 1 << LDE_LOG_BLOWUP, a.shape[0], _offset(form))
    else:
        exp = O.evaluate_fft(O.F_STARK252, a, 1, a.shape[0], _offset(form))
    assert exp.shape == (1 << log_n, 4)
    if log_n <= _CACHE_UP_TO:
        exp.setflags(write=False)
        _expecteds[key] = exp
    return exp


def _run(form, log_n, a, batch):
    """`a`: batch blocks of input elements, densely packed.  Returns the batch outputs, densely packed."""
    import torch
    from lambda_elliptic_curves_amd import fft
    fld = util.field_pairs()["stark252"][0]
    t_in = torch.from_numpy(np.array(a).view(np.int64)).cuda()   # a copy: the shared inputs are read-only
    t_out = torch.full((batch << log_n, 4), POISON, dtype=torch.int64, device="cuda")
    if form == "lde":
        fft.lde_device(fld, t_in, log_n - LDE_LOG_BLOWUP, t_out, log_n, batch=batch, offset=_offset(form))
    else:
        fft.ntt_device(fld, t_in, t_out, log_n, inverse=form in ("inverse", "coset-inverse"), batch=batch,
                       batch_stride=1 << log_n, offset=_offset(form))
    torch.cuda.synchronize()
    return t_out.cpu().numpy().view(np.uint64)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("log_n", SIZES)
def test_matches_oracle(log_n, form, kind):
    got = _run(form, log_n, _input(kind, _in_log(form, log_n)), 1)
    assert np.array_equal(got, _expected(kind, log_n, form))


@pytest.mark.parametrize("first", range(len(KINDS)), ids=KINDS)
@pytest.mark.parametrize("form", FORMS)
def test_batch_of_three_2_16(form, first):
    """three different inputs in one launch: `first` and the two kinds after it"""
    kinds = [KINDS[(first + b) % len(KINDS)] for b in range(3)]
    a = np.concatenate([_input(k, _in_log(form, 16)) for k in kinds])
    got = _run(form, 16, a, 3)
    for b, k in enumerate(kinds):
        assert np.array_equal(got[b << 16:(b + 1) << 16], _expected(k, 16, form)), (b, k)
