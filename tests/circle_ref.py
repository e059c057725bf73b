"""Circle FFT over Mersenne31, restated from the definitions (math/src/circle/ of the reference): the circle group, the
standard coset, the twiddles, the layered transforms in plain integers and in numpy, and the naive evaluation in the
basis {1, y, x, xy, 2x^2 - 1, ...}.  No size limit of its own (the reference's coset points stop at 2^8)."""
import numpy as np

P = (1 << 31) - 1
GENERATOR = (2, 1268011823)   # of the whole circle group, order 2^31


def reduce_word(w):
    """A u32 read the way from_base_type reads it, then brought to the canonical residue."""
    w = int(w)
    return ((w & P) + (w >> 31)) % P


def inv(a):
    return pow(a, P - 2, P)


# ---- the circle group {(x, y): x^2 + y^2 = 1}
def padd(a, b):
    return ((a[0] * b[0] - a[1] * b[1]) % P, (a[0] * b[1] + a[1] * b[0]) % P)


def pdouble(a):
    return ((2 * a[0] * a[0] - 1) % P, (2 * a[0] * a[1]) % P)


def pmul(k, a):
    r = (1, 0)
    while k:
        if k & 1:
            r = padd(r, a)
        a = pdouble(a)
        k >>= 1
    return r


def subgroup_generator(log2_order):
    """g_{2^k} = 2^(31 - k) * G"""
    g = GENERATOR
    for _ in range(31 - log2_order):
        g = pdouble(g)
    return g


def coset_points(log2n):
    """The standard coset of size n: g_{2n} + i * g_n, i = 0 .. n - 1."""
    shift, step = subgroup_generator(log2n + 1), subgroup_generator(log2n)
    pts, cur = [], shift
    for _ in range(1 << log2n):
        pts.append(cur)
        cur = padd(cur, step)
    return pts


# ---- twiddles
def get_twiddles(log2n, interpolation=False):
    """The layers as the reference builds them: y of the half coset, x of its first half, then x -> 2x^2 - 1 on the
    first half of the previous layer.  Evaluation: reversed (lengths 1, 2, .., n/2).  Interpolation: the inverses, in
    the order built (lengths n/2, .., 1)."""
    n = 1 << log2n
    shift, step = subgroup_generator(log2n + 1), subgroup_generator(log2n - 1) if log2n > 1 else (1, 0)
    half, cur = [], shift
    for _ in range(n // 2):   # half coset: same shift, step g_{n/2}
        half.append(cur)
        cur = padd(cur, step)
    layers = [[q[1] for q in half]]
    if log2n >= 2:
        layers.append([q[0] for q in half[: len(half) // 2]])
        for _ in range(log2n - 2):
            prev = layers[-1]
            layers.append([(2 * x * x - 1) % P for x in prev[: len(prev) // 2]])
    if interpolation:
        return [[inv(t) for t in layer] for layer in layers]
    return layers[::-1]


def twiddle_closed_form(log2n, i, j):
    """tw[i][j] of the evaluation order: x((1 + 4j) g_{2^(i+3)}) below the last layer, y((1 + 4j) g_{2^(L+1)}) in it."""
    if i < log2n - 1:
        return pmul(1 + 4 * j, subgroup_generator(i + 3))[0]
    return pmul(1 + 4 * j, subgroup_generator(log2n + 1))[1]


def flat_twiddles(log2n, config):
    """What lw_circle_get_twiddles writes: the layers of get_twiddles concatenated, n - 1 words."""
    return np.array([t for layer in get_twiddles(log2n, bool(config)) for t in layer], np.uint32)


# ---- permutations
def bit_reverse(v):
    n = len(v)
    bits = n.bit_length() - 1
    return [v[int(format(i, "0%db" % bits)[::-1], 2) if bits else 0] for i in range(n)]


def order_result(a):
    n = len(a)
    out = [0] * n
    for i in range(n // 2):
        out[2 * i] = a[i]
        out[2 * i + 1] = a[n - 1 - i]
    return out


def order_input(e):
    return list(e[0::2]) + list(e[1::2][::-1])


# ---- layered transforms, plain integers
def evaluate_cfft(coeffs):
    a = bit_reverse([reduce_word(c) for c in coeffs])
    n = len(a)
    L = n.bit_length() - 1
    tw = get_twiddles(L)
    for i in range(L):
        h = 1 << i
        for s in range(0, n, 2 * h):
            for j in range(h):
                hi, t = a[s + j], a[s + h + j] * tw[i][j] % P
                a[s + j], a[s + h + j] = (hi + t) % P, (hi - t) % P
    return order_result(a)


def interpolate_cfft(evals):
    if len(evals) == 0:
        return []
    a = order_input([reduce_word(e) for e in evals])
    n = len(a)
    L = n.bit_length() - 1
    tw = get_twiddles(L, True)
    for i in range(L):
        h = 1 << (L - i - 1)
        for s in range(0, n, 2 * h):
            for j in range(h):
                hi, lo = a[s + j], a[s + h + j]
                a[s + j], a[s + h + j] = (hi + lo) % P, (hi - lo) * tw[i][j] % P
    ninv = inv(n % P)
    return [c * ninv % P for c in bit_reverse(a)]


# ---- naive evaluation in the basis
def basis_value(k, x, y):
    v = y if k & 1 else 1
    k >>= 1
    while k:
        if k & 1:
            v = v * x % P
        x = (2 * x * x - 1) % P
        k >>= 1
    return v


def evaluate_naive(coeffs):
    n = len(coeffs)
    L = n.bit_length() - 1
    c = [reduce_word(w) for w in coeffs]
    return [sum(c[k] * basis_value(k, x, y) for k in range(n)) % P for (x, y) in coset_points(L)]


# ---- the same layers in numpy (uint64 products of two 31-bit values), for sizes up to 2^22
def _np_reduce_words(w):
    w = np.asarray(w, np.uint64) & np.uint64(0xFFFFFFFF)
    return ((w & np.uint64(P)) + (w >> np.uint64(31))) % np.uint64(P)


def _np_bitrev_index(L):
    idx = np.arange(1 << L, dtype=np.uint64)
    rev = np.zeros_like(idx)
    for b in range(L):
        rev |= ((idx >> np.uint64(b)) & np.uint64(1)) << np.uint64(L - 1 - b)
    return rev.astype(np.int64)


_NP_TW = {}


def np_twiddles(L):
    """(evaluation layers, interpolation layers) as uint64 arrays; built layer by layer from the points, cached."""
    if L in _NP_TW:
        return _NP_TW[L]
    p = np.uint64(P)
    n = 1 << L
    half = n // 2
    # half coset by doubling: points[k] = shift + k * step; built with the block rule pts[m + k] = pts[k] + m * step
    shift, step = subgroup_generator(L + 1), subgroup_generator(L - 1) if L > 1 else (1, 0)
    xs = np.array([shift[0]], np.uint64)
    ys = np.array([shift[1]], np.uint64)
    mstep = step
    while len(xs) < half:
        sx, sy = np.uint64(mstep[0]), np.uint64(mstep[1])
        nx = (xs * sx % p + (p - ys * sy % p)) % p
        ny = (xs * sy % p + ys * sx % p) % p
        xs, ys = np.concatenate([xs, nx]), np.concatenate([ys, ny])
        mstep = pdouble(mstep)
    layers = [ys]
    if L >= 2:
        layers.append(xs[: half // 2])
        for _ in range(L - 2):
            prev = layers[-1][: len(layers[-1]) // 2]
            layers.append((np.uint64(2) * (prev * prev % p) % p + p - np.uint64(1)) % p)

    def np_inv(a):   # a^(p - 2)
        r = np.ones_like(a)
        b, e = a.copy(), P - 2
        while e:
            if e & 1:
                r = r * b % p
            b = b * b % p
            e >>= 1
        return r
    res = (layers[::-1], [np_inv(layer) for layer in layers])
    _NP_TW[L] = res
    return res


def np_evaluate_cfft(coeffs):
    """coeffs: (..., n) words; returns canonical residues as uint32."""
    p = np.uint64(P)
    a = _np_reduce_words(coeffs)
    n = a.shape[-1]
    L = n.bit_length() - 1
    lead = a.shape[:-1]
    a = a[..., _np_bitrev_index(L)]
    tw = np_twiddles(L)[0]
    for i in range(L):
        h = 1 << i
        v = a.reshape(lead + (n // (2 * h), 2, h))
        hi, t = v[..., 0, :], v[..., 1, :] * tw[i] % p
        a = np.stack([(hi + t) % p, (hi + p - t) % p], axis=-2).reshape(lead + (n,))
    out = np.empty_like(a)
    out[..., 0::2] = a[..., : n // 2]
    out[..., 1::2] = a[..., ::-1][..., : n // 2]
    return out.astype(np.uint32)


def np_interpolate_cfft(evals):
    p = np.uint64(P)
    e = _np_reduce_words(evals)
    n = e.shape[-1]
    L = n.bit_length() - 1
    lead = e.shape[:-1]
    a = np.concatenate([e[..., 0::2], e[..., 1::2][..., ::-1]], axis=-1)
    tw = np_twiddles(L)[1]
    for i in range(L):
        h = 1 << (L - i - 1)
        v = a.reshape(lead + (n // (2 * h), 2, h))
        hi, lo = v[..., 0, :], v[..., 1, :]
        a = np.stack([(hi + lo) % p, (hi + p - lo) % p * tw[i] % p], axis=-2).reshape(lead + (n,))
    a = a[..., _np_bitrev_index(L)]
    return (a * np.uint64(inv(n % P)) % p).astype(np.uint32)


def np_lde(evals, log2_out):
    c = np_interpolate_cfft(evals)
    pad = np.zeros(c.shape[:-1] + ((1 << log2_out) - c.shape[-1],), np.uint32)
    return np_evaluate_cfft(np.concatenate([c, pad], axis=-1))
