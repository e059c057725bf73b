"""GPU parity for scalars of 1 to 8 u64 limbs (lw_hip_msm_limbs[_device], msm(..., scalar_limbs=L)) against the oracle with
the same k_limbs.  The reference's Pippenger is generic over the width, msm<const NUM_LIMBS, G> (math/src/msm/
pippenger.rs:18-32); its own property test runs on UnsignedInteger<6> (pippenger.rs:181-233).  The sum is over the full
integers: points outside the prime-order subgroup tell that apart from a reduction mod r.  Equality is on the affine image."""
import ctypes as C

import numpy as np
import pytest

from oracle import bigint_def as D
from oracle import oracle as O
from tests import util

pytestmark = pytest.mark.gpu
CURVES = ["bls12_381_g1", "bn254_g1", "bn254_g2", "bls12_381_g2"]
BLS = O.C_BLS12_381_G1


def aff(oid, p):
    return O.point_to_affine_ints(oid, p)


def rand_limbs(rng, n, limbs):
    """n uniform integers of 64 * limbs bits as (n, limbs) u64 rows, most significant limb first"""
    return np.frombuffer(rng.bytes(8 * n * limbs), dtype=np.uint64).reshape(n, limbs).copy()


def widen(s, limbs):
    """(n, k) rows -> (n, limbs) rows of the same integers (zero limbs in front: MS limb first)"""
    return np.concatenate([np.zeros((s.shape[0], limbs - s.shape[1]), np.uint64), s], axis=1)


@pytest.mark.parametrize("seed", range(20))
def test_reference_property_test_on_six_limb_scalars(seed):
    """pippenger.rs:204-233: msm == naive and msm_with(window) == naive for windows 1..7 on UnsignedInteger<6> scalars and
    points G * power for random u128 powers, n in [0, 30)."""
    from lambda_elliptic_curves_amd import msm
    rng = np.random.default_rng(0x6C1B + seed)
    n = int(rng.integers(0, 30))
    cs = rand_limbs(rng, n, 6)
    g = util.generator(BLS)
    pts = np.stack([O.ec_mul(BLS, g, int.from_bytes(rng.bytes(16), "big"), 2) for _ in range(n)]) if n else np.zeros((0, 18), np.uint64)
    exp = aff(BLS, O.msm_naive(BLS, cs, pts, k_limbs=6))
    got = msm.msm(msm.BLS12381Curve, cs, pts, scalar_limbs=6)
    assert aff(BLS, got) == exp
    if n == 0:
        assert exp is None
    for window in range(1, 8):
        assert aff(BLS, O.msm_with(BLS, cs, pts, window, k_limbs=6)) == exp
        assert aff(BLS, msm.msm_with(msm.BLS12381Curve, cs, pts, window, scalar_limbs=6)) == exp


def _points_outside_subgroup(count, seed):
    """BLS12-381 G1 points from random x: y = (x^3 + 4)^((p+1)/4) (p = 3 mod 4), kept when [r]P != O"""
    c = D.BLS12_381_G1
    p, r = D.P_FP381, D.P_FR381
    rng = np.random.default_rng(seed)
    out = []
    while len(out) < count:
        x = int.from_bytes(rng.bytes(48), "big") % p
        rhs = (x * x * x + 4) % p
        y = pow(rhs, (p + 1) // 4, p)
        if y * y % p != rhs:
            continue
        if c.mul(r, c.pt(x, y)) is None:
            continue
        out.append(O.point_from_affine_ints(BLS, x, y))
    return np.stack(out)


def test_full_integer_sum_outside_the_prime_order_subgroup():
    from lambda_elliptic_curves_amd import msm
    n = 12                                 # (the affine [r]P check in pure Python takes about a second per point)
    pts = _points_outside_subgroup(n, 0xC0F)
    rng = np.random.default_rng(0xC0F)
    r = D.P_FR381
    ks = [int.from_bytes(rng.bytes(16), "big") * r + int.from_bytes(rng.bytes(32), "big") % r for _ in range(n)]
    ks[0] = r                              # r * P != O outside the subgroup
    ks[1] = (1 << 384) - 1
    cs = O.ints_to_array(ks, 6)
    exp = aff(BLS, O.msm(BLS, cs, pts, k_limbs=6))
    got = msm.msm(msm.BLS12381Curve, cs, pts, scalar_limbs=6)
    assert aff(BLS, got) == exp
    reduced = O.ints_to_array([k % r for k in ks], 4)
    assert aff(BLS, O.msm(BLS, reduced, pts)) != exp, "the inputs do not tell the full sum from the reduced one"
    assert aff(BLS, msm.msm(msm.BLS12381Curve, reduced, pts)) != aff(BLS, got)


def _special_scalars(limbs):
    B = 64 * limbs
    out = [(1 << B) - 1, 1 << (B - 1), (1 << (B - 1)) - 1, 0, 1, 2, 1 << (B // 2), (1 << (B // 2)) - 1]
    for c in range(3, 21):   # every digit 2^(c-1): the largest that does not carry; and 2^(c-1) + 1: the smallest that does
        out.append(sum((1 << (c - 1)) << (c * w) for w in range(B // c)))
        out.append(sum(((1 << (c - 1)) + 1) << (c * w) for w in range(B // c)) & ((1 << B) - 1))
    return out


@pytest.mark.parametrize("limbs", [1, 2, 3, 5, 6, 8])
@pytest.mark.parametrize("name,n", [("bls12_381_g1", 3000), ("bn254_g1", 2000), ("bn254_g2", 500), ("bls12_381_g2", 400)])
def test_every_window_width_and_limb_count_matches_oracle(name, n, limbs, monkeypatch):
    """LW_HIP_MSM_C over 3..20 (the split top window where c divides 64 L: c = 4, 8, 16 and more), with all-ones scalars
    that carry through every window into the top one, zero scalars, identity rows and P next to -P."""
    from lambda_elliptic_curves_amd import msm
    crv, oid = util.curve_pairs()[name]
    _, points = util.msm_case(oid, n, 4100 + n + limbs)
    rng = np.random.default_rng(n * 10 + limbs)
    cs = rand_limbs(rng, n, limbs)
    special = _special_scalars(limbs)
    ks = O.ints_to_array(special, limbs)
    for i in range(len(special)):
        cs[(i * 7) % n] = ks[i]
    cs[n - 10:n - 5] = 0                                # zero scalars
    points[3] = O.ec_neutral(oid)                        # identity rows, with a non-zero scalar
    points[4] = O.ec_neutral(oid)
    points[11] = O.ec_neg(oid, points[10])               # P and -P with the same scalar: they cancel
    cs[11] = cs[10]
    points[13] = O.ec_neg(oid, points[12])               # P and -P with all-ones scalars
    cs[12] = cs[13] = np.uint64(0xFFFFFFFFFFFFFFFF)
    exp = aff(oid, O.parallel_msm_with(oid, cs, points, 8, util.host_threads(), k_limbs=limbs))
    for c in range(3, 21):
        monkeypatch.setenv("LW_HIP_MSM_C", str(c))
        assert aff(oid, msm.msm(crv, cs, points, scalar_limbs=limbs)) == exp, f"L = {limbs}, c = {c}"


@pytest.mark.parametrize("limbs", [1, 2, 6, 8])
def test_all_scalars_equal_fill_one_bucket(limbs, monkeypatch):
    from lambda_elliptic_curves_amd import msm
    crv, oid = util.curve_pairs()["bls12_381_g1"]
    n = 2500
    _, points = util.msm_case(oid, n, 4400 + limbs)
    for v in ((1 << (64 * limbs)) - 1, 0x9E3779B97F4A7C15 << (64 * limbs - 64)):
        cs = np.tile(O.ints_to_array([v], limbs), (n, 1))
        exp = aff(oid, O.msm(oid, cs, points, k_limbs=limbs))
        for c in (3, 8, 13, 16, 20):
            monkeypatch.setenv("LW_HIP_MSM_C", str(c))
            assert aff(oid, msm.msm(crv, cs, points, scalar_limbs=limbs)) == exp, f"L = {limbs}, c = {c}"


@pytest.mark.parametrize("name,n", [("bls12_381_g1", 5000), ("bn254_g1", 1 << 19), ("bn254_g2", 600)])
def test_zero_extension_agrees_with_the_four_limb_call(name, n):
    from lambda_elliptic_curves_amd import _lib, msm
    crv, oid = util.curve_pairs()[name]
    s4, points = util.msm_case(oid, n, 4500 + n, threads=util.host_threads())
    s4[0] = np.uint64(0xFFFFFFFFFFFFFFFF)                 # 2^256 - 1: the top window of the 4-limb split
    ref4 = aff(oid, msm.msm(crv, s4, points))
    for limbs in (5, 6, 8):                               # zero top limbs
        assert aff(oid, msm.msm(crv, widen(s4, limbs), points, scalar_limbs=limbs)) == ref4, f"L = {limbs}"
    rng = np.random.default_rng(n)
    for limbs in (1, 2):                                  # narrow scalars widened to 4 limbs through lw_hip_msm
        s = rand_limbs(rng, n, limbs)
        s[1] = np.uint64(0xFFFFFFFFFFFFFFFF)
        assert aff(oid, msm.msm(crv, s, points, scalar_limbs=limbs)) == aff(oid, msm.msm(crv, widen(s, 4), points)), f"L = {limbs}"
    # scalar_limbs = 4 is the same call as lw_hip_msm, byte for byte
    L = _lib.lib()
    a = np.zeros(crv.point_words, np.uint64)
    b = np.zeros(crv.point_words, np.uint64)
    vp = lambda x: x.ctypes.data_as(C.c_void_p)   # noqa: E731
    assert L.lw_hip_msm(crv.curve, vp(s4), n, vp(points), n, vp(a)) == 0
    assert L.lw_hip_msm_limbs(crv.curve, vp(s4), 4, n, vp(points), n, vp(b)) == 0
    assert a.tobytes() == b.tobytes()


def _scale_case(name, log_n, limbs, seed):
    import torch
    from lambda_elliptic_curves_amd import msm
    crv, oid = util.curve_pairs()[name]
    n = 1 << log_n
    thr = util.host_threads()
    _, points = util.msm_case(oid, n, seed, threads=thr)
    cs = rand_limbs(np.random.default_rng(seed), n, limbs)
    ts = torch.from_numpy(cs.view(np.int64)).cuda()
    tp = torch.from_numpy(points.view(np.int64)).cuda()
    got = msm.msm_device(crv, ts, tp, n, scalar_limbs=limbs)
    del ts, tp
    torch.cuda.empty_cache()
    exp = O.parallel_msm_with(oid, cs, points, max(2, O.optimum_window_size(n)), thr, k_limbs=limbs)
    assert aff(oid, got) == aff(oid, exp)
    return crv, oid, cs, points, got


@pytest.mark.parametrize("name,log_n,limbs", [("bls12_381_g1", 24, 6), ("bn254_g1", 23, 2), ("bls12_381_g2", 18, 6)])
def test_device_resident_at_scale_matches_oracle(name, log_n, limbs):
    _scale_case(name, log_n, limbs, 4600 + log_n)


def test_host_buffer_call_equals_device_resident_call_2_21():
    from lambda_elliptic_curves_amd import msm
    crv, oid, cs, points, got = _scale_case("bls12_381_g1", 21, 6, 4721)
    host = msm.msm(crv, cs, points, scalar_limbs=6)
    assert aff(oid, host) == aff(oid, got)
