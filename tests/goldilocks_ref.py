"""The Goldilocks NTT restated in Python integers (and in numpy uint64 for the larger sizes): what the GPU tests of
lambda_elliptic_curves_amd/goldilocks.py compare against.  Follows math/src/fft/ of the reference over U64TestField
(p = 2^64 - 2^32 + 1): evaluate_fft / interpolate_fft and the offset forms, the NR-DIT layers of cpu/fft.rs:20-55 with
bit-reversed twiddles, get_twiddles of cpu/roots_of_unity.rs, and reduce_128 of u64_goldilocks_field.rs:187-203."""
import numpy as np

P = (1 << 64) - (1 << 32) + 1
EPS = (1 << 32) - 1
M64 = (1 << 64) - 1
TWO_ADICITY = 32
ROOT = 1753635133440165772            # TWO_ADIC_PRIMITVE_ROOT_OF_UNITY = 7^((p - 1) / 2^32)
OTHER_ROOT = 7277203076849721926      # another primitive 2^32-th root
assert ROOT == pow(7, (P - 1) >> 32, P)

# operands that take every branch of reduce_128 (and of an add / sub with wrap) many times; all below p
EDGE = [0, 1, 2, 3, 7, 1 << 31, (1 << 32) - 2, (1 << 32) - 1, 1 << 32, (1 << 32) + 1, 1 << 33, (1 << 33) - 1, 1 << 48,
        (1 << 63) - 1, 1 << 63, (1 << 63) + 1, (P - 1) // 2, (P + 1) // 2, 0x0000FFFF0000FFFF, 0x8000000080000000,
        0xFFFF0000FFFF0000, P - (1 << 48), P - (1 << 32) - 1, P - (1 << 32), P - 3, P - 2, P - 1, ROOT]
assert len(EDGE) == 28 and all(0 <= v < P for v in EDGE)
EDGE_PAIRS = [(a, b) for a in EDGE for b in EDGE]


def reduce_word(w):
    """from_base_type: any u64, x >= p means x - p."""
    return w - P if w >= P else w


def is_primitive_root(g):
    return 0 < g < P and pow(g, 1 << 31, P) == P - 1


def root_of_unity(order, root=ROOT):
    """get_primitive_root_of_unity (traits.rs:82-94)."""
    assert order <= TWO_ADICITY
    return pow(root, 1 << (TWO_ADICITY - order), P)


def bitrev(x, bits):
    r = 0
    for _ in range(bits):
        r = (r << 1) | (x & 1)
        x >>= 1
    return r


def reduce_128(x):
    """reduce_128 line by line; returns (residue, borrow branch taken, carry branch taken, result was >= p before the final
    conditional subtraction)."""
    x_lo, x_hi = x & M64, x >> 64
    x_hi_hi, x_hi_lo = x_hi >> 32, x_hi & EPS
    t0 = (x_lo - x_hi_hi) & M64
    borrow = x_lo < x_hi_hi
    if borrow:
        t0 = (t0 - EPS) & M64
    t1 = x_hi_lo * EPS
    t2 = t0 + t1
    carry = t2 > M64
    t2 &= M64
    if carry:
        t2 = t2 + EPS
        assert t2 <= M64
    over = t2 >= P
    return (t2 - P if over else t2), borrow, carry, over


# ---- the transforms in Python integers
def evaluate_naive(coeffs, offset=1, root=ROOT):
    n = len(coeffs)
    L = n.bit_length() - 1
    w, h = root_of_unity(L, root), offset % P
    out = []
    for i in range(n):
        x, acc = h * pow(w, i, P) % P, 0
        for c in reversed(coeffs):
            acc = (acc * x + c) % P
        out.append(acc)
    return out


def twiddles_bitrev(L, root=ROOT, inverse=False):
    """T[g] = w^bitrev(g), g < n / 2: get_twiddles(L, BitReverse[Inversed])."""
    w = root_of_unity(L, root)
    if inverse:
        w = pow(w, P - 2, P)
    return [pow(w, bitrev(g, L - 1), P) for g in range((1 << L) // 2)]


def nr_dit(values, tw):
    """in_place_nr_2radix_fft: natural order in, bit-reversed order out."""
    a = [reduce_word(v) for v in values]
    n = len(a)
    group_count, group_size = 1, n
    while group_count < n:
        half = group_size // 2
        for g in range(group_count):
            first = g * group_size
            w = tw[g]
            for i in range(first, first + half):
                wi = w * a[i + half] % P
                a[i], a[i + half] = (a[i] + wi) % P, (a[i] - wi) % P
        group_count, group_size = group_count * 2, half
    return a


def bit_reverse_permute(a):
    bits = len(a).bit_length() - 1
    return [a[bitrev(i, bits)] for i in range(len(a))]


def evaluate_fft(coeffs, offset=None, root=ROOT):
    """The layered form: scale by h^i, NR-DIT, bit reverse."""
    n = len(coeffs)
    L = n.bit_length() - 1
    a = [reduce_word(v) for v in coeffs]
    if offset is not None:
        h = offset % P
        a = [c * pow(h, i, P) % P for i, c in enumerate(a)]
    if L == 0:
        return a
    return bit_reverse_permute(nr_dit(a, twiddles_bitrev(L, root)))


def interpolate_fft(evals, offset=None, root=ROOT):
    n = len(evals)
    L = n.bit_length() - 1
    a = [reduce_word(v) for v in evals]
    if L > 0:
        a = bit_reverse_permute(nr_dit(a, twiddles_bitrev(L, root, True)))
    ninv = pow(n, P - 2, P)
    a = [v * ninv % P for v in a]
    if offset is not None:
        hinv = pow(offset % P, P - 2, P)
        a = [c * pow(hinv, i, P) % P for i, c in enumerate(a)]
    return a


def lde(coeffs, log2n, offset=None, root=ROOT):
    """evaluate_offset_fft(poly, blowup, Some(domain), offset): scale, zero pad, transform."""
    a = [reduce_word(v) for v in coeffs]
    if offset is not None:
        h = offset % P
        a = [c * pow(h, i, P) % P for i, c in enumerate(a)]
    return evaluate_fft(a + [0] * ((1 << log2n) - len(a)), None, root)


def get_twiddles(order, config, root=ROOT):
    """RootsConfig 0 Natural, 1 NaturalInversed, 2 BitReverse, 3 BitReverseInversed: 2^order / 2 entries."""
    count = (1 << order) // 2
    if count == 0:
        return []
    w = root_of_unity(order, root)
    if config & 1:
        w = pow(w, P - 2, P)
    nat = [pow(w, i, P) for i in range(count)]
    return nat if config < 2 else bit_reverse_permute(nat)


# ---- numpy uint64, the product split into 32-bit halves
_EPS = np.uint64(EPS)
_P = np.uint64(P)
_S32 = np.uint64(32)


def np_reduce(a):
    a = np.asarray(a, np.uint64)
    return np.where(a >= _P, a - _P, a)


def np_add(a, b):
    s = a + b
    return np.where((s < a) | (s >= _P), s + _EPS, s)


def np_sub(a, b):
    d = a - b
    return np.where(a < b, d - _EPS, d)


def np_mul(a, b):
    a, b = np.asarray(a, np.uint64), np.asarray(b, np.uint64)
    al, ah, bl, bh = a & _EPS, a >> _S32, b & _EPS, b >> _S32
    ll = al * bl
    mid = al * bh + (ll >> _S32)
    mid2 = ah * bl + (mid & _EPS)
    x_hi = ah * bh + (mid >> _S32) + (mid2 >> _S32)
    x_lo = (mid2 << _S32) | (ll & _EPS)
    hh, hl = x_hi >> _S32, x_hi & _EPS
    t0 = x_lo - hh
    t0 = np.where(x_lo < hh, t0 - _EPS, t0)
    t1 = (hl << _S32) - hl
    t2 = t0 + t1
    t2 = np.where(t2 < t1, t2 + _EPS, t2)
    return np.where(t2 >= _P, t2 - _P, t2)


def _np_powers(base, count):
    """base^0 .. base^(count - 1) by doubling."""
    out = np.ones(count, np.uint64)
    have, step = 1, np.array([base % P], np.uint64)
    while have < count:
        m = min(have, count - have)
        out[have:have + m] = np_mul(out[:m], step)
        have += m
        step = np_mul(step, step)
    return out


def _np_bitrev_index(L):
    idx = np.arange(1 << L, dtype=np.uint64)
    r = np.zeros(1 << L, np.uint64)
    for _ in range(L):
        r = (r << np.uint64(1)) | (idx & np.uint64(1))
        idx >>= np.uint64(1)
    return r.astype(np.int64)


def _np_transform(a, L, w):
    """(batch, n) canonical words -> the transform with root w, natural order in and out."""
    n = 1 << L
    if L == 0:
        return a
    tw = _np_powers(w, n // 2)[_np_bitrev_index(L - 1)] if L > 1 else np.ones(1, np.uint64)
    a = a.copy()
    groups = 1
    while groups < n:
        v = a.reshape(a.shape[0], groups, 2, n // (2 * groups))
        t = np_mul(v[:, :, 1, :], tw[:groups].reshape(1, groups, 1))
        lo = v[:, :, 0, :].copy()
        v[:, :, 0, :] = np_add(lo, t)
        v[:, :, 1, :] = np_sub(lo, t)
        groups *= 2
    return a[:, _np_bitrev_index(L)]


def np_evaluate_fft(coeffs, offset=None, root=ROOT, log2n=None):
    """Rows of `coeffs` (or one row) -> their evaluations; log2n > log2(len): the low-degree extension."""
    c = np.asarray(coeffs, np.uint64)
    a = np_reduce(np.atleast_2d(c))
    Lc = a.shape[1].bit_length() - 1
    L = Lc if log2n is None else log2n
    if offset is not None:
        a = np_mul(a, _np_powers(offset, a.shape[1]).reshape(1, -1))
    if L > Lc:
        a = np.concatenate([a, np.zeros((a.shape[0], (1 << L) - (1 << Lc)), np.uint64)], axis=1)
    out = _np_transform(a, L, root_of_unity(L, root))
    return out[0] if c.ndim == 1 else out


def np_interpolate_fft(evals, offset=None, root=ROOT):
    e = np.asarray(evals, np.uint64)
    a = np_reduce(np.atleast_2d(e))
    L = a.shape[1].bit_length() - 1
    out = _np_transform(a, L, pow(root_of_unity(L, root), P - 2, P))
    out = np_mul(out, np.array([pow(1 << L, P - 2, P)], np.uint64))
    if offset is not None:
        out = np_mul(out, _np_powers(pow(offset % P, P - 2, P), 1 << L).reshape(1, -1))
    return out[0] if e.ndim == 1 else out
