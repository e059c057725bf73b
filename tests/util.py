"""Shared helpers for the parity tests: seeded inputs in the reference's memory layout."""
import numpy as np

from oracle import oracle as O

# (product Field, oracle field id)
def field_pairs():
    from lambda_elliptic_curves_amd import fft
    return {
        "stark252": (fft.Stark252PrimeField, O.F_STARK252),
        "fr381": (fft.FrField, O.F_FR381),
        "babybear_u64": (fft.Babybear31PrimeField, O.F_BABYBEAR_U64),
        "babybear_u32": (fft.Babybear31PrimeFieldU32, O.F_BABYBEAR_U32),
        "babybear_ext4": (fft.Degree4BabyBearExtensionField, O.F_BABYBEAR_EXT4),
    }


def fld(name):
    """the product Field of a name"""
    return field_pairs()[name][0]


P_BABYBEAR = 2013265921


def field_modulus(name):
    from oracle import bigint_def as D
    return {"stark252": D.P_STARK252, "fr381": D.P_FR381}.get(name, P_BABYBEAR)


def rand_elems(name, n, seed):
    """n canonical residues (any value < p is a valid Montgomery-form element), reference layout."""
    rng = np.random.default_rng(seed)
    if name in ("stark252", "fr381"):
        a = rng.integers(0, 1 << 63, size=(n, 4), dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, size=(n, 4), dtype=np.uint64)
        top_bits = 59 if name == "stark252" else 62      # 2^251 < p_stark, 2^254 < p_fr381
        a[:, 0] &= np.uint64((1 << top_bits) - 1)
        return a
    if name == "babybear_u32":
        return rng.integers(0, P_BABYBEAR, size=n, dtype=np.uint32)
    if name == "babybear_u64":
        return rng.integers(0, P_BABYBEAR, size=n, dtype=np.uint64)
    if name == "babybear_ext4":
        return rng.integers(0, P_BABYBEAR, size=(n, 4), dtype=np.uint64)
    raise KeyError(name)


def to_ints(a):
    """stored 256-bit elements, (n, 4) uint64 MS limb first -> Python integers"""
    a = np.ascontiguousarray(a, dtype=np.uint64).reshape(-1, 4)
    b = a.astype(">u8").tobytes()
    return [int.from_bytes(b[32 * i:32 * i + 32], "big") for i in range(a.shape[0])]


def to_arr(vals):
    """Python integers below 2^256 -> (n, 4) uint64, MS limb first"""
    if not len(vals):
        return np.zeros((0, 4), np.uint64)
    b = b"".join(int(v).to_bytes(32, "big") for v in vals)
    return np.frombuffer(b, dtype=">u8").astype(np.uint64).reshape(-1, 4)


def dev(arr):
    """a (n, 4) uint64 array -> an int64 tensor on the device (a copy: read-only arrays are welcome)"""
    import torch
    return torch.from_numpy(np.ascontiguousarray(arr).view(np.int64).copy()).cuda()


def host(t):
    return t.cpu().numpy().view(np.uint64)


def offset_elem(name, h):
    """Coset offset h (small canonical int) as one domain-field element in memory form."""
    base = {"babybear_ext4": "babybear_u64"}.get(name, name)
    oid = field_pairs()[base][1]
    return O.elems_to_mont(oid, [h])[0] if oid != O.F_BABYBEAR_U32 else O.elems_to_mont(oid, [h])[:1]


def curve_pairs():
    from lambda_elliptic_curves_amd import msm
    return {
        "bls12_381_g1": (msm.BLS12381Curve, O.C_BLS12_381_G1),
        "bn254_g1": (msm.BN254Curve, O.C_BN254_G1),
        "bn254_g2": (msm.BN254TwistCurve, O.C_BN254_G2),
        "bls12_381_g2": (msm.BLS12381TwistCurve, O.C_BLS12_381_G2),
    }


def generator(oid):
    from oracle import bigint_def as D
    c = D.CURVES[oid]
    return O.point_from_affine_ints(oid, c.gen[0].tup(), c.gen[1].tup())


def msm_case(oid, n, seed, threads=1):
    """Synthetic MSM input: uniform 256-bit canonical scalars, SRS-like projective points
    P_i = [s0 + i*delta]G — n DISTINCT points — built by repeated projective addition (so Z != 1), from a fixed seed.
    threads > 1 builds the run in `threads` pieces concurrently (piece t starts at [s0 + t*chunk*delta]G): the same
    group elements, different projective representatives at the piece boundaries."""
    rng = np.random.default_rng(seed)
    scalars = rng.integers(0, 1 << 63, size=(n, 4), dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, size=(n, 4), dtype=np.uint64)
    s0 = int(rng.integers(1, 1 << 62))
    delta = int(rng.integers(1, 1 << 62))
    g = generator(oid)
    if threads <= 1 or n < 4 * threads:
        return scalars, O.gen_points(oid, g, s0, delta, n)
    from concurrent.futures import ThreadPoolExecutor
    chunk = (n + threads - 1) // threads
    spans = [(t * chunk, min(n, (t + 1) * chunk)) for t in range(threads) if t * chunk < n]
    with ThreadPoolExecutor(len(spans)) as ex:   # ctypes releases the GIL inside the C call
        parts = list(ex.map(lambda ab: O.gen_points(oid, g, s0 + ab[0] * delta, delta, ab[1] - ab[0]), spans))
    return scalars, np.concatenate(parts)


def host_threads(cap=16):
    """Worker threads for the CPU checker on this box (the GPU box gives a one-GPU job 16 cores)."""
    import os
    return max(1, min(cap, os.cpu_count() or 1))


def stone_compat_trace_columns(initial, n):
    """Fibonacci2ColsShifted trace (provers/stark/src/examples/fibonacci_2_cols_shifted.rs:249-265) as two columns of
    canonical integers: col0[0] = 1, col1[0] = initial, (x, y) -> (y, x + y)."""
    from oracle import bigint_def as D
    p = D.P_STARK252
    x, y = 1, initial % p
    c0, c1 = [x], [y]
    for _ in range(1, n):
        x, y = y, (x + y) % p
        c0.append(x)
        c1.append(y)
    return c0, c1


def plonk_test_srs(oid, length, secret=2):
    """test_srs (provers/plonk/src/test_utils/utils.rs:32-44): [secret^i]G1, i < length, projective, via the oracle."""
    from oracle import bigint_def as D
    g = generator(oid)
    r = D.P_FR381
    return np.stack([O.ec_mul(oid, g, pow(secret, i, r), 4) for i in range(length)])


def groth16_h_by_composition(l, r, o, gates):
    """calculate_h_coefficients (provers/groth16/src/qap.rs:15-39) as a composition of oracle transforms and Python
    big-integer pointwise arithmetic — the independent check of O.groth16_h_coefficients at small sizes."""
    from oracle import bigint_def as D
    f = O.F_FR381
    off = O.elems_to_mont(f, [7])[0]
    deg = 2 * gates
    le, re_, oe = (O.evaluate_fft(f, x, 1, deg, off) for x in (l, r, o))
    p = D.P_FR381
    coeffs = [p - 1] + [0] * (gates - 1) + [1]       # t_poly = x^gates - 1 (qap.rs:21-25), then batch inverse
    t = O.evaluate_fft(f, O.elems_to_mont(f, coeffs), 1, deg, off)
    lc, rc, oc, tc = (O.elems_from_mont(f, x) for x in (le, re_, oe, t))
    h = [((a * b - c) * pow(d, -1, p)) % p for a, b, c, d in zip(lc, rc, oc, tc)]
    return O.interpolate_fft(f, O.elems_to_mont(f, h), off, strip=True)


# ---- device-resident NTT cases shared by test_gpu_ntt.py and test_gpu_ntt_babybear.py: every buffer is a 2-d array of
# the layout's words, one row per element
def ntt_words(name, a):
    return np.ascontiguousarray(a).reshape(np.shape(a)[0], -1)


def ntt_columns(name, count, n, seed):
    """`count` columns of n elements each, (count, n, words); the last coefficient of each is not zero, so that
    Polynomial::new strips nothing"""
    a = ntt_words(name, rand_elems(name, count * n, seed))
    a = a.reshape(count, n, a.shape[1]).copy()
    a[:, -1, -1] |= a.dtype.type(1)
    return a


def ntt_oracle(name, col, inverse=False, offset=None, log2n=None):
    """one column through the oracle: evaluate_[offset_]fft (zero padded to 2^log2n if given) or interpolate_[offset_]fft"""
    oid = field_pairs()[name][1]
    col = col.reshape(-1) if name == "babybear_u32" else col
    if inverse:
        out = O.interpolate_fft(oid, col, offset)
    elif log2n is None:
        out = O.evaluate_fft(oid, col, 1, None, offset)
    else:
        out = O.evaluate_fft(oid, col, 1, 1 << log2n, offset)
    out = ntt_words(name, out)
    assert out.shape[0] == (col.shape[0] if log2n is None else 1 << log2n)
    return out


def _to_device(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int32 if a.dtype == np.uint32 else np.int64).copy()).cuda()


def ntt_on_device(name, a, log2n, batch, stride=0, inverse=False, offset=None, out=None, lde_from=None):
    """lw_hip_ntt_device on device copies of `a` and `out` (None: in place), or lw_hip_ntt_lde_device from dense blocks of
    2^lde_from coefficients; returns (the output buffer, the input buffer afterwards) as arrays like `out` and `a`"""
    import torch
    from lambda_elliptic_curves_amd import fft
    fld = field_pairs()[name][0]
    t_in = _to_device(a)
    t_out = t_in if out is None else _to_device(out)
    if lde_from is None:
        fft.ntt_device(fld, t_in, t_out, log2n, inverse=inverse, batch=batch, batch_stride=stride, offset=offset)
    else:
        fft.lde_device(fld, t_in, lde_from, t_out, log2n, batch=batch, offset=offset)
    torch.cuda.synchronize()
    like = a if out is None else out
    return t_out.cpu().numpy().view(like.dtype).reshape(like.shape), t_in.cpu().numpy().view(a.dtype).reshape(a.shape)


SPLIT_BATCH = 32768 + 3   # grid.y carries at most 32768 columns: a chunk of 32768 and one of 3
_NTT_SPLIT = {}


def ntt_split_case(name):
    """SPLIT_BATCH columns of 2^1 elements that cycle through four distinct inputs, and what the oracle makes of them
    under offset 3: forward, inverse and extended to 2^2.  Computed once per field and left unchanged."""
    if name not in _NTT_SPLIT:
        four = ntt_columns(name, 4, 2, 1500)
        off = offset_elem(name, 3)
        tile = lambda cols: np.concatenate([cols[b % 4] for b in range(SPLIT_BATCH)])
        case = {"off": off, "in": tile(four)}
        for key, kw in (("fwd", {}), ("inv", {"inverse": True}), ("lde", {"log2n": 2})):
            outs = [ntt_oracle(name, c, offset=off, **kw) for c in four]
            assert len({o.tobytes() for o in outs}) == 4   # a chunk offset that is off by one cannot hide behind equal columns
            case[key] = tile(outs)
        for v in case.values():
            v.setflags(write=False)
        _NTT_SPLIT[name] = case
    return _NTT_SPLIT[name]


def check_ntt_split(name, inverse, in_place):
    """SPLIT_BATCH columns of the smallest transform, one pass: in place is the copy through the work buffer, per chunk"""
    case = ntt_split_case(name)
    a = case["in"]
    got, after = ntt_on_device(name, a, 1, SPLIT_BATCH, inverse=inverse, offset=case["off"], out=None if in_place else np.zeros_like(a))
    assert got.tobytes() == case["inv" if inverse else "fwd"].tobytes()
    assert in_place or after.tobytes() == a.tobytes()


def check_ntt_lde_split(name):
    """dense blocks of 2^1 coefficients into 2^2 evaluations each: past the split the input advances by 2, the output by 4"""
    case = ntt_split_case(name)
    a = case["in"]
    got, after = ntt_on_device(name, a, 2, SPLIT_BATCH, offset=case["off"], out=np.zeros((2 * a.shape[0], a.shape[1]), a.dtype), lde_from=1)
    assert got.tobytes() == case["lde"].tobytes() and after.tobytes() == a.tobytes()


def check_ntt_strided(name, log2n):
    """3 columns, n + 8 elements apart, canaries between them and behind the last: forward, inverse, coset forward and
    coset inverse, into a second buffer and in place.  One pass up to 2^8 (in place: the staging copy), two from 2^9 on
    (BabyBear at 2^13 and 2^16: the kernels with the tile shape compiled in)."""
    n, batch = 1 << log2n, 3
    stride = n + 8
    cols = ntt_columns(name, batch, n, 1600 + log2n)
    W, dt = cols.shape[2], cols.dtype
    canary = dt.type(0xDEADBEEF if dt == np.uint32 else 0xDEADBEEFCAFEF00D)
    a = np.full((batch, stride, W), canary, dt)
    a[:, :n] = cols
    a = a.reshape(batch * stride, W)
    off = offset_elem(name, 3)
    for inverse, offset in ((False, None), (True, None), (False, off), (True, off)):
        want = np.full((batch, stride, W), canary, dt)
        for b in range(batch):
            want[b, :n] = ntt_oracle(name, cols[b], inverse=inverse, offset=offset)
        want = want.reshape(batch * stride, W)
        got, after = ntt_on_device(name, a, log2n, batch, stride, inverse=inverse, offset=offset, out=np.full_like(a, canary))
        assert got.tobytes() == want.tobytes() and after.tobytes() == a.tobytes(), (inverse, offset is not None, "distinct")
        got, _ = ntt_on_device(name, a, log2n, batch, stride, inverse=inverse, offset=offset)
        assert got.tobytes() == want.tobytes(), (inverse, offset is not None, "in place")
