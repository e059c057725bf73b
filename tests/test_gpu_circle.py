"""GPU parity of the circle FFT over Mersenne31 (csrc/circle.hip) with the restatement of math/src/circle/ in
tests/circle_ref.py: equality of canonical residues, which is what the reference's PartialEq compares.

Pass counts (ceil(L / 8) passes of at most 8 layers): one pass up to 2^8, two from 2^9, three from 2^17, four from 2^25.
The four-pass plan is reached at 2^14 with LW_HIP_CIRCLE_MAX_R=4 (honoured under LW_HIP_TUNING, which tests/conftest.py
sets), which also gives a three-pass plan at 2^9 and 2^12."""
import json
import os

import numpy as np
import pytest

from tests import circle_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = R.P
GOLDEN = json.load(open(os.path.join(ROOT, "tests", "golden", "circle_m31.json")))


def words(shape, seed):
    """any u32, a few of them the awkward ones"""
    w = np.random.default_rng(seed).integers(0, 1 << 32, shape, dtype=np.uint64).astype(np.uint32)
    flat = w.reshape(-1)
    for k, v in enumerate((P, 0, 1 << 31, 0xFFFFFFFF, P - 1)):
        flat[(k * 7919) % flat.size] = v
    return w


def to_dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int32).copy()).cuda()


def to_host(t):
    return t.cpu().numpy().view(np.uint32)


def dev_transform(a, inverse, **kw):
    import torch
    from lambda_elliptic_curves_amd import circle
    a = np.atleast_2d(a)
    t_in = to_dev(a)
    t_out = torch.empty_like(t_in)
    f = circle.interpolate_cfft_device if inverse else circle.evaluate_cfft_device
    f(t_in, t_out, a.shape[1].bit_length() - 1, batch=a.shape[0], **kw)
    torch.cuda.synchronize()
    return to_host(t_out)


class max_r:
    """LW_HIP_CIRCLE_MAX_R for the duration of a block (read per call)"""

    def __init__(self, r):
        self.r = r

    def __enter__(self):
        if self.r:
            os.environ["LW_HIP_CIRCLE_MAX_R"] = str(self.r)

    def __exit__(self, *exc):
        os.environ.pop("LW_HIP_CIRCLE_MAX_R", None)


def test_golden_vectors_host_and_device():
    from lambda_elliptic_curves_amd import circle
    for case in GOLDEN["evaluations"]:
        c, e = np.array(case["coeffs"], np.uint32), np.array(case["evals"], np.uint32)
        assert np.array_equal(circle.evaluate_cfft(c), e) and np.array_equal(circle.interpolate_cfft(e), c)
        assert np.array_equal(dev_transform(c, False)[0], e) and np.array_equal(dev_transform(e, True)[0], c)
    for case in GOLDEN["roundtrips"]:
        c = np.array(case["coeffs"], np.uint32)
        assert np.array_equal(circle.interpolate_cfft(circle.evaluate_cfft(c)), c)
        assert np.array_equal(dev_transform(dev_transform(c, False), True)[0], c)
        assert np.array_equal(circle.evaluate_cfft(c), np.array(R.evaluate_cfft(case["coeffs"]), np.uint32))


# 1 .. 8 one pass, 9 the first two-pass size, 9 .. 14 every register-step shape of a short last pass (tile 2^13: through 14),
# 16 the last two-pass size, 17 the first three-pass size
@pytest.mark.parametrize("L", list(range(1, 15)) + [16, 17])
def test_parity_with_the_restatement(L):
    from lambda_elliptic_curves_amd import circle
    w = words((2, 1 << L), 300 + L)
    ev, co = R.np_evaluate_cfft(w), R.np_interpolate_cfft(w)
    assert np.array_equal(dev_transform(w, False), ev)
    assert np.array_equal(dev_transform(w, True), co)
    if L <= 12:   # the host form
        assert np.array_equal(circle.evaluate_cfft(w), ev) and np.array_equal(circle.interpolate_cfft(w[0]), co[0])


@pytest.mark.parametrize("L,r", [(9, 4), (12, 4), (14, 4), (14, 5)])   # 3, 3, 4 (the plan of 2^25 .. 2^30) and 3 passes
def test_parity_at_the_higher_pass_counts(L, r):
    w = words((2, 1 << L), 400 + L)
    with max_r(r):
        ev, co = dev_transform(w, False), dev_transform(w, True)
    assert np.array_equal(ev, R.np_evaluate_cfft(w)) and np.array_equal(co, R.np_interpolate_cfft(w))


def test_parity_at_2_20():
    w = words((1, 1 << 20), 20)
    assert np.array_equal(dev_transform(w, False), R.np_evaluate_cfft(w))
    assert np.array_equal(dev_transform(w, True), R.np_interpolate_cfft(w))


@pytest.mark.parametrize("L", [3, 8, 10])
def test_edge_words(L):
    n = 1 << L
    cases = [np.full(n, v, np.uint64).astype(np.uint32) for v in (0, 1, P - 1, P, 1 << 31, 0xFFFFFFFF)]
    for at in (0, n - 1, n // 2):
        v = np.zeros(n, np.uint32)
        v[at] = P - 1
        cases.append(v)
    w = np.stack(cases)
    reduced = np.array([[R.reduce_word(x) for x in row] for row in w], np.uint32)
    for inverse, ref in ((False, R.np_evaluate_cfft), (True, R.np_interpolate_cfft)):
        got = dev_transform(w, inverse)
        assert (got < P).all()
        assert np.array_equal(got, dev_transform(reduced, inverse)) and np.array_equal(got, ref(w))


def test_interpolate_inverts_evaluate_at_2_16():
    w = words((1, 1 << 16), 16)
    back = dev_transform(dev_transform(w, False), True)
    assert np.array_equal(back[0], np.array([R.reduce_word(x) for x in w[0]], np.uint32))


@pytest.mark.parametrize("L", [1, 2, 3, 10])
def test_get_twiddles(L):
    from lambda_elliptic_curves_amd import circle
    for config in (circle.TWIDDLES_EVALUATION, circle.TWIDDLES_INTERPOLATION):
        got, exp = circle.get_twiddles(L, config), R.get_twiddles(L, bool(config))
        assert [layer.tolist() for layer in got] == exp


@pytest.mark.parametrize("L", [7, 11])   # one pass, two passes
@pytest.mark.parametrize("inverse", [False, True])
def test_batch_stride_and_canary(L, inverse):
    import torch
    from lambda_elliptic_curves_amd import circle
    n, stride, canary = 1 << L, (1 << L) + 5, np.uint32(0xDEADBEEF)
    w = words((3, n), 700 + L)
    buf = np.full(3 * stride, canary, np.uint32)
    for k in range(3):
        buf[k * stride:k * stride + n] = w[k]
    f = circle.interpolate_cfft_device if inverse else circle.evaluate_cfft_device
    t_in = to_dev(buf)
    t_out = to_dev(np.full(3 * stride, canary, np.uint32))
    f(t_in, t_out, L, batch=3, batch_stride=stride)
    torch.cuda.synchronize()
    out = to_host(t_out)
    exp = (R.np_interpolate_cfft if inverse else R.np_evaluate_cfft)(w)
    for k in range(3):
        assert np.array_equal(out[k * stride:k * stride + n], exp[k])
        assert (out[k * stride + n:(k + 1) * stride] == canary).all()
    assert np.array_equal(to_host(t_in), buf)
    assert np.array_equal(dev_transform(w, inverse, batch_stride=0), exp)   # stride 0 is the contiguous form
    assert np.array_equal(dev_transform(w, inverse, batch_stride=n), exp)


@pytest.mark.parametrize("L", [6, 12])   # one pass, two passes
@pytest.mark.parametrize("inverse", [False, True])
def test_in_place(L, inverse):
    import torch
    from lambda_elliptic_curves_amd import circle
    w = words((2, 1 << L), 800 + L)
    t = to_dev(w)
    (circle.interpolate_cfft_device if inverse else circle.evaluate_cfft_device)(t, t, L, batch=2)
    torch.cuda.synchronize()
    assert np.array_equal(to_host(t), dev_transform(w, inverse))
    assert np.array_equal(to_host(t), (R.np_interpolate_cfft if inverse else R.np_evaluate_cfft)(w))


@pytest.mark.parametrize("lin,lout", [(1, 1), (1, 4), (6, 8), (10, 13), (12, 16)])
def test_lde(lin, lout):
    import torch
    from lambda_elliptic_curves_amd import circle
    w = words((2, 1 << lin), 900 + lout)
    t_in = to_dev(w)
    t_out = torch.empty((2, 1 << lout), dtype=torch.int32, device="cuda")
    circle.lde_device(t_in, lin, t_out, lout, batch=2)
    torch.cuda.synchronize()
    assert np.array_equal(to_host(t_out), R.np_lde(w, lout))
    assert np.array_equal(to_host(t_in), w)
    if lin == lout:   # the input reduced mod p
        assert np.array_equal(to_host(t_out), np.array([[R.reduce_word(x) for x in row] for row in w], np.uint32))


def test_lde_strided():
    import torch
    from lambda_elliptic_curves_amd import circle
    lin, lout, canary = 5, 9, np.uint32(0xDEADBEEF)
    sin, sout = (1 << lin) + 3, (1 << lout) + 7
    w = words((2, 1 << lin), 950)
    buf = np.full(2 * sin, canary, np.uint32)
    for k in range(2):
        buf[k * sin:k * sin + (1 << lin)] = w[k]
    t_in, t_out = to_dev(buf), to_dev(np.full(2 * sout, canary, np.uint32))
    circle.lde_device(t_in, lin, t_out, lout, batch=2, in_stride=sin, out_stride=sout)
    torch.cuda.synchronize()
    out, exp = to_host(t_out), R.np_lde(w, lout)
    for k in range(2):
        assert np.array_equal(out[k * sout:k * sout + (1 << lout)], exp[k])
        assert (out[k * sout + (1 << lout):(k + 1) * sout] == canary).all()


def test_non_default_stream():
    import torch
    from lambda_elliptic_curves_amd import circle
    L = 12
    w = words((1, 1 << L), 1200)
    s = torch.cuda.Stream()
    t_in = to_dev(w)
    t_out = torch.empty_like(t_in)
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        circle.evaluate_cfft_device(t_in, t_out, L, stream=s.cuda_stream)
    s.synchronize()   # that stream alone
    assert np.array_equal(to_host(t_out), R.np_evaluate_cfft(w))


def test_warm_cache_smaller_and_larger_sizes():
    # the shared x-table and the per-size y-tables under reuse: 2^12 warms both, 2^5 is served by a prefix of the x-table
    # and a y-table of its own, 2^18 has to grow the x-table, and 2^12 afterwards must still be right
    for L in (12, 5, 18, 12, 5):
        w = words((1, 1 << L), 1300 + L)
        assert np.array_equal(dev_transform(w, False), R.np_evaluate_cfft(w))
        assert np.array_equal(dev_transform(w, True), R.np_interpolate_cfft(w))


SPLIT_BATCH = 32768 + 3   # grid.y carries at most 32768 columns: a chunk of 32768 and one of 3
_SPLIT = {}


def split_case():
    """the columns and both references, computed once"""
    if not _SPLIT:
        w = words((SPLIT_BATCH, 2), 1400)
        marked = (0, 32767, 32768, SPLIT_BATCH - 1)   # either side of the chunk boundary and both ends
        for k, col in enumerate(marked):
            w[col] = (11 + k, 101 + 7 * k)
        _SPLIT.update(w=w, ev=R.np_evaluate_cfft(w), co=R.np_interpolate_cfft(w))
        for exp in (_SPLIT["ev"], _SPLIT["co"]):   # a chunk offset that is off by one cannot hide behind equal columns
            assert len({tuple(exp[col]) for col in marked} | {tuple(exp[1]), tuple(exp[32766]), tuple(exp[32769])}) == 7
    return _SPLIT


@pytest.mark.parametrize("in_place", [False, True])
@pytest.mark.parametrize("inverse", [False, True])
def test_batch_split_above_32768_columns(inverse, in_place):
    # 2^1 words per column, the smallest size: one pass, so in place is the copy through the work buffer, per chunk
    import torch
    from lambda_elliptic_curves_amd import circle
    case = split_case()
    t_in = to_dev(case["w"])
    t_out = t_in if in_place else torch.zeros_like(t_in)
    (circle.interpolate_cfft_device if inverse else circle.evaluate_cfft_device)(t_in, t_out, 1, batch=SPLIT_BATCH)
    torch.cuda.synchronize()
    assert np.array_equal(to_host(t_out), case["co" if inverse else "ev"])
    if not in_place:
        assert np.array_equal(to_host(t_in), case["w"])


def test_lde_batch_split_above_32768_columns():
    # 2^1 evaluations into 2^2 per column, strided on both sides: past the split the input advances by its own stride
    import torch
    from lambda_elliptic_curves_amd import circle
    four = words((4, 2), 1500)
    exp4 = R.np_lde(four, 2)
    assert len({tuple(r) for r in exp4}) == 4
    sin, sout, canary = 3, 5, np.uint32(0xDEADBEEF)
    pick = np.arange(SPLIT_BATCH) % 4
    buf = np.full((SPLIT_BATCH, sin), canary, np.uint32)
    buf[:, :2] = four[pick]
    exp = np.full((SPLIT_BATCH, sout), canary, np.uint32)
    exp[:, :4] = exp4[pick]
    t_in, t_out = to_dev(buf.reshape(-1)), to_dev(np.full(SPLIT_BATCH * sout, canary, np.uint32))
    circle.lde_device(t_in, 1, t_out, 2, batch=SPLIT_BATCH, in_stride=sin, out_stride=sout)
    torch.cuda.synchronize()
    assert np.array_equal(to_host(t_out).reshape(SPLIT_BATCH, sout), exp)
    assert np.array_equal(to_host(t_in).reshape(SPLIT_BATCH, sin), buf)
