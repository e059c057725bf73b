"""Goldilocks NTT on the device against tests/goldilocks_ref.py: canonical words, bit for bit.

Sizes.  The tile is 2^12 words and a pass runs at most 8 stages, so one pass serves 2^0 .. 2^8 (register steps 1, 2, 3, 4,
3+2, 3+3, 4+3, 4+4 stages: every shape of a short last pass), two passes 2^9 .. 2^16 (2^12 is the first size with full tiles,
2^13 the first with more than one block per pass) and 2^17 is the first three-pass size.  Four passes (2^25 under the
default plan) are reached at 2^14 with LW_HIP_GOLDILOCKS_MAX_R=4, honoured under LW_HIP_TUNING, which tests/conftest.py sets.

The product gl_mul is plain C++ shared by the host and the device; its rare branches are reached by the operand pairs
EDGE x EDGE only (goldilocks_ref.py), here through the pointwise product, the coset load and the butterfly."""
import os

import numpy as np
import pytest

from tests import goldilocks_ref as R

pytestmark = pytest.mark.gpu
P = R.P
U64 = (1 << 64) - 1


def _gl():
    from lambda_elliptic_curves_amd import goldilocks
    return goldilocks


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint64).view(np.int64).copy()).cuda()


def _host(t):
    return t.cpu().numpy().view(np.uint64)


def _rand(shape, seed):
    """any u64 words, some of them at and above p"""
    w = np.random.default_rng(seed).integers(0, 1 << 64, shape, dtype=np.uint64)
    flat = w.reshape(-1)
    flat[::7] = np.uint64(U64)
    flat[3::11] = np.uint64(P)
    return w


def _ntt(a, log2n, inverse=False, batch=1, stride=0, offset=None, root=0, in_place=False):
    import torch
    t_in = _dev(a)
    t_out = t_in if in_place else torch.zeros_like(t_in)
    _gl().ntt_device(t_in, t_out, log2n, inverse=inverse, batch=batch, batch_stride=stride, offset=offset, root=root)
    torch.cuda.synchronize()
    return _host(t_out)


def _ref(a, inverse=False, offset=None, root=R.ROOT):
    return (R.np_interpolate_fft if inverse else R.np_evaluate_fft)(a, offset, root)


class _MaxR:
    """LW_HIP_GOLDILOCKS_MAX_R for the duration of a block (read per call)"""

    def __init__(self, r):
        self.r = r

    def __enter__(self):
        os.environ["LW_HIP_GOLDILOCKS_MAX_R"] = str(self.r)

    def __exit__(self, *exc):
        os.environ.pop("LW_HIP_GOLDILOCKS_MAX_R", None)


@pytest.mark.parametrize("L", list(range(0, 15)) + [16, 17])
def test_pass_structure(L):
    a = _rand((2, 1 << L), 300 + L)
    for inverse in (False, True):
        got = _ntt(a, L, inverse=inverse, batch=2)
        assert np.array_equal(got, _ref(a, inverse)), (L, inverse)
    if L <= 8:   # the numpy form against the integers once more, on the device's own input
        assert got[0].tolist() == R.interpolate_fft([int(v) for v in a[0]])


@pytest.mark.parametrize("L,max_r,passes", [(9, 4, 3), (12, 4, 3), (14, 4, 4), (14, 5, 3)])
def test_higher_pass_counts(L, max_r, passes):
    assert -(-L // max_r) == passes
    a = _rand((2, 1 << L), 400 + L + max_r)
    with _MaxR(max_r):
        fwd = _ntt(a, L, batch=2)
        inv = _ntt(a, L, inverse=True, batch=2, offset=7)
        t_out = _dev(np.zeros((2, 1 << L), np.uint64))
        _gl().lde_device(_dev(a[:, :1 << (L - 2)]), L - 2, t_out, L, batch=2, offset=7)
    assert np.array_equal(fwd, _ref(a))
    assert np.array_equal(inv, _ref(a, True, 7))
    assert np.array_equal(_host(t_out), R.np_evaluate_fft(a[:, :1 << (L - 2)], 7, log2n=L))


def test_one_large_size():
    a = _rand(1 << 20, 20)
    ev = _ntt(a, 20)
    assert np.array_equal(ev, _ref(a))
    assert np.array_equal(_ntt(ev, 20, inverse=True), R.np_reduce(a))


def test_device_multiplier_edges():
    import torch
    a = np.array([x for x, _ in R.EDGE_PAIRS], np.uint64)
    b = np.array([y for _, y in R.EDGE_PAIRS], np.uint64)
    want = np.array([x * y % P for x, y in R.EDGE_PAIRS], np.uint64)
    ta, tb = _dev(a), _dev(b)
    t_out = torch.zeros_like(ta)
    _gl().mul_device(ta, tb, t_out)
    torch.cuda.synchronize()
    assert np.array_equal(_host(t_out), want)
    _gl().mul_device(ta, tb, ta)   # out aliases a
    torch.cuda.synchronize()
    assert np.array_equal(_host(ta), want) and np.array_equal(_host(tb), b)
    # words at and above p on either side mean their residues
    big = np.array([P, P + 1, U64, U64], np.uint64)
    other = np.array([5, P - 1, U64, P + 7], np.uint64)
    t_big = _dev(big)
    _gl().mul_device(t_big, _dev(other), t_big)
    torch.cuda.synchronize()
    assert _host(t_big).tolist() == [int(x) % P * (int(y) % P) % P for x, y in zip(big, other)]


def test_device_multiplier_edges_through_the_coset_load():
    # for each pair (a, h): the forward transform of (0, a) with offset h at log2n = 1 is (a h, -a h)
    import torch
    for h in R.EDGE:
        if h == 0:
            continue   # a zero offset is an error (test_goldilocks_cpu.py)
        cols = np.array([[0, a] for a in R.EDGE], np.uint64)
        got = _ntt(cols, 1, batch=len(R.EDGE), offset=h)
        assert got.tolist() == [[a * h % P, -a * h % P] for a in R.EDGE], h
    # the butterfly's sum and difference over the same pairs (a + b wraps in 210 of them), times 2^-1 on the store
    half = pow(2, P - 2, P)
    cols = np.array([[a, b] for a, b in R.EDGE_PAIRS], np.uint64)
    got = _ntt(cols, 1, inverse=True, batch=len(R.EDGE_PAIRS))
    assert got.tolist() == [[(a + b) * half % P, (a - b) * half % P] for a, b in R.EDGE_PAIRS]


@pytest.mark.parametrize("L", [3, 8, 10])
def test_edge_words_through_the_transform(L):
    n = 1 << L
    rows = [[v] * n for v in (0, 1, P - 1, P, P + 1, 1 << 63, U64)]
    for at in (0, n // 2, n - 1):
        v = [0] * n
        v[at] = P - 1
        rows.append(v)
    a = np.array(rows, np.uint64)
    reduced = R.np_reduce(a)
    for inverse in (False, True):
        got = _ntt(a, L, inverse=inverse, batch=len(rows))
        assert (got < np.uint64(P)).all()
        assert np.array_equal(got, _ntt(reduced, L, inverse=inverse, batch=len(rows)))
        assert np.array_equal(got, _ref(a, inverse))
    assert got[1].tolist() == R.interpolate_fft(rows[1]) and got[-1].tolist() == R.interpolate_fft(rows[-1])


@pytest.mark.parametrize("L", [1, 7, 11, 17])
def test_coset(L):
    a = _rand((2, 1 << L), 500 + L)
    for h in (7, P - 1, 1 << 32):
        assert np.array_equal(_ntt(a, L, batch=2, offset=h), _ref(a, False, h)), h
        assert np.array_equal(_ntt(a, L, inverse=True, batch=2, offset=h), _ref(a, True, h)), h


def test_coset_inverse_of_forward():
    a = _rand(1 << 16, 16)
    ev = _ntt(a, 16, offset=7)
    assert np.array_equal(_ntt(ev, 16, inverse=True, offset=7), R.np_reduce(a))
    assert np.array_equal(_ntt(a, 16, offset=P + 7), ev)   # the offset is read mod p too


@pytest.mark.parametrize("lc,L", [(0, 0), (0, 3), (1, 4), (6, 8), (10, 13), (12, 16)])
def test_lde(lc, L):
    import torch
    c = _rand((2, 1 << lc), 600 + L)
    for h in (None, 7):
        t_c = _dev(c)
        t_out = torch.zeros((2, 1 << L), dtype=torch.int64, device="cuda")
        _gl().lde_device(t_c, lc, t_out, L, batch=2, offset=h)
        torch.cuda.synchronize()
        assert np.array_equal(_host(t_out), R.np_evaluate_fft(c, h, log2n=L)), h
        assert np.array_equal(_host(t_c), c)   # the input is unchanged
    if L <= 4:
        assert _host(t_out)[0].tolist() == R.lde([int(v) for v in c[0]], L, 7)


def test_lde_strided_with_canaries():
    import torch
    lc, L, sin, sout, batch = 5, 9, 40, 600, 3
    canary = np.uint64(0xDEADBEEFCAFEF00D)
    c = np.full(batch * sin, canary, np.uint64)
    cols = _rand((batch, 1 << lc), 77)
    for b in range(batch):
        c[b * sin:b * sin + (1 << lc)] = cols[b]
    out = np.full(batch * sout, canary, np.uint64)
    t_c, t_out = _dev(c), _dev(out)
    _gl().lde_device(t_c, lc, t_out, L, batch=batch, in_stride=sin, out_stride=sout, offset=7)
    torch.cuda.synchronize()
    got = _host(t_out).reshape(batch, sout)
    assert np.array_equal(got[:, :1 << L], R.np_evaluate_fft(cols, 7, log2n=L))
    assert (got[:, 1 << L:] == canary).all() and np.array_equal(_host(t_c), c)


@pytest.mark.parametrize("L", [7, 11])
def test_batch_stride_with_canaries(L):
    n, batch = 1 << L, 3
    stride = n + 24
    canary = np.uint64(0xDEADBEEFCAFEF00D)
    cols = _rand((batch, n), 700 + L)
    a = np.full((batch, stride), canary, np.uint64)
    a[:, :n] = cols
    for inverse in (False, True):
        want = _ref(cols, inverse)
        got = _ntt(a.reshape(-1), L, inverse=inverse, batch=batch, stride=stride).reshape(batch, stride)
        assert np.array_equal(got[:, :n], want) and (got[:, n:] == 0).all()   # the gaps of the zeroed output stay as they were
        again = _ntt(a.reshape(-1), L, inverse=inverse, batch=batch, stride=stride, in_place=True).reshape(batch, stride)
        assert np.array_equal(again[:, :n], want) and (again[:, n:] == canary).all()
        assert np.array_equal(_ntt(cols, L, inverse=inverse, batch=batch, stride=0), _ntt(cols, L, inverse=inverse, batch=batch, stride=n))
        host = _gl().ntt(a.reshape(-1), inverse=inverse, log2n=L, batch=batch, batch_stride=stride).reshape(batch, stride)
        assert np.array_equal(host[:, :n], want) and (host[:, n:] == canary).all()


@pytest.mark.parametrize("L", [6, 12])
def test_in_place(L):
    a = _rand((2, 1 << L), 800 + L)
    for inverse in (False, True):
        assert np.array_equal(_ntt(a, L, inverse=inverse, batch=2, in_place=True), _ref(a, inverse))
    assert np.array_equal(_ntt(a, L, batch=2, offset=7, in_place=True), _ref(a, False, 7))


@pytest.mark.parametrize("order", [0, 1, 2, 3, 10])
def test_get_twiddles(order):
    for config in range(4):
        got = _gl().get_twiddles(order, config)
        assert got.dtype == np.uint64 and got.tolist() == R.get_twiddles(order, config), (order, config)
    assert _gl().get_twiddles(order, 2, root=R.OTHER_ROOT).tolist() == R.get_twiddles(order, 2, R.OTHER_ROOT)


def test_non_default_root_rebuilds_the_cache_both_ways():
    a = _rand(1 << 10, 10)
    first = _ntt(a, 10)
    other = _ntt(a, 10, root=R.OTHER_ROOT)
    assert np.array_equal(other, _ref(a, root=R.OTHER_ROOT)) and not np.array_equal(other, first)
    assert np.array_equal(_ntt(other, 10, inverse=True, root=R.OTHER_ROOT), R.np_reduce(a))
    assert np.array_equal(_ntt(a, 10), first) and np.array_equal(first, _ref(a))
    assert np.array_equal(_ntt(a, 10, root=R.ROOT), first)   # the default root spelled out is the same cache entry


def test_warm_cache():
    for L in (12, 5, 18, 12, 5):
        a = _rand(1 << L, 900 + L)
        assert np.array_equal(_ntt(a, L), _ref(a)), L
        assert np.array_equal(_ntt(a, L, inverse=True), _ref(a, True)), L


def test_non_default_stream():
    import torch
    a = _rand((2, 1 << 13), 13)
    s = torch.cuda.Stream()
    t_in = _dev(a)
    t_out = torch.zeros_like(t_in)
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        _gl().ntt_device(t_in, t_out, 13, batch=2, offset=7)
    _gl().ntt_device(t_out, t_out, 13, inverse=True, batch=2, offset=7, stream=s.cuda_stream)
    s.synchronize()
    assert np.array_equal(_host(t_out), R.np_reduce(a))


def test_host_forms():
    G = _gl()
    c = _rand(5, 55)
    c[3], c[4] = np.uint64(12345), np.uint64(P)   # a trailing zero, spelled p: stripped
    ev = G.evaluate_fft(c, blowup_factor=2, domain_size=6)
    assert ev.shape == (16,) and ev.tolist() == R.lde([int(v) for v in c[:4]], 4)
    ev7 = G.evaluate_offset_fft(c, 4, None, 7)
    assert ev7.shape == (16,) and ev7.tolist() == R.lde([int(v) for v in c[:4]], 4, 7)
    back = G.interpolate_fft(ev, strip=True)
    assert back.tolist() == [R.reduce_word(int(v)) for v in c[:4]]
    assert G.interpolate_offset_fft(ev7, 7).tolist() == [R.reduce_word(int(v)) for v in c[:4]] + [0] * 12
    a = _rand(64, 64)
    assert G.ntt(a).tolist() == R.evaluate_fft([int(v) for v in a])
    assert G.ntt(a, inverse=True, offset=3, root=R.OTHER_ROOT).tolist() == R.interpolate_fft([int(v) for v in a], 3, R.OTHER_ROOT)
    # the polynomial product the pointwise kernel is for: (1 + 2x)(3 + x) = 3 + 7x + 2x^2
    import torch
    fa, fb = _dev(G.evaluate_fft(np.array([1, 2], np.uint64), 2)), _dev(G.evaluate_fft(np.array([3, 1], np.uint64), 2))
    G.mul_device(fa, fb, fa)
    torch.cuda.synchronize()
    assert G.interpolate_fft(_host(fa), strip=True).tolist() == [3, 7, 2]


SPLIT_BATCH = 32768 + 3   # grid.y carries at most 32768 columns: a chunk of 32768 and one of 3
_SPLIT = {}


def _split_case():
    """the columns and both references (coset offset 7), computed once"""
    if not _SPLIT:
        a = _rand((SPLIT_BATCH, 2), 1000)
        marked = (0, 32767, 32768, SPLIT_BATCH - 1)   # either side of the chunk boundary and both ends
        for k, col in enumerate(marked):
            a[col] = (11 + k, 101 + 7 * k)
        _SPLIT.update(a=a, fwd=_ref(a, False, 7), inv=_ref(a, True, 7))
        for exp in (_SPLIT["fwd"], _SPLIT["inv"]):   # a chunk offset that is off by one cannot hide behind equal columns
            assert len({tuple(exp[col]) for col in marked} | {tuple(exp[1]), tuple(exp[32766]), tuple(exp[32769])}) == 7
    return _SPLIT


@pytest.mark.parametrize("in_place", [False, True])
@pytest.mark.parametrize("inverse", [False, True])
def test_batch_split_above_32768_columns(inverse, in_place):
    # 2^1 words per column: one pass, so in place is the copy through the work buffer, per chunk
    case = _split_case()
    got = _ntt(case["a"], 1, inverse=inverse, batch=SPLIT_BATCH, offset=7, in_place=in_place)
    assert np.array_equal(got, case["inv" if inverse else "fwd"])


def test_lde_batch_split_above_32768_columns():
    # 2^1 coefficients into 2^2 evaluations per column, strided on both sides: past the split the input advances by its own stride
    import torch
    four = _rand((4, 2), 1100)
    exp4 = R.np_evaluate_fft(four, 7, log2n=2)
    assert len({tuple(r) for r in exp4}) == 4
    sin, sout, canary = 3, 5, np.uint64(0xDEADBEEFCAFEF00D)
    pick = np.arange(SPLIT_BATCH) % 4
    buf = np.full((SPLIT_BATCH, sin), canary, np.uint64)
    buf[:, :2] = four[pick]
    exp = np.full((SPLIT_BATCH, sout), canary, np.uint64)
    exp[:, :4] = exp4[pick]
    t_c, t_out = _dev(buf.reshape(-1)), _dev(np.full(SPLIT_BATCH * sout, canary, np.uint64))
    _gl().lde_device(t_c, 1, t_out, 2, batch=SPLIT_BATCH, in_stride=sin, out_stride=sout, offset=7)
    torch.cuda.synchronize()
    assert np.array_equal(_host(t_out).reshape(SPLIT_BATCH, sout), exp)
    assert np.array_equal(_host(t_c).reshape(SPLIT_BATCH, sin), buf)
