"""GPU parity for the device-resident affine SRS (lw_hip_srs_* / lw_hip_msm_srs): the same group element as
msm(cs, points[:len(cs)]) — checked against the CPU oracle's Pippenger (math/src/msm/pippenger.rs:18-103) and against
the projective HIP path, including the cases only a mixed-addition path can get wrong (identity rows in the SRS,
P and -P, repeated points, everything in one bucket)."""
import numpy as np
import pytest

from oracle import bigint_def as D
from oracle import oracle as O
from tests import util

pytestmark = pytest.mark.gpu
CURVES = ["bls12_381_g1", "bn254_g1", "bn254_g2", "bls12_381_g2"]


def aff(oid, p):
    return O.point_to_affine_ints(oid, p)


@pytest.mark.parametrize("name", CURVES)
@pytest.mark.parametrize("n", [1, 2, 17, 100, 1000])
def test_srs_msm_matches_reference_algorithm(name, n):
    from lambda_elliptic_curves_amd import msm
    crv, oid = util.curve_pairs()[name]
    scalars, points = util.msm_case(oid, n, 300 + n)
    srs = msm.Srs(crv, points)
    got = srs.msm(scalars)
    exp = O.msm(oid, scalars, points)
    assert aff(oid, got) == aff(oid, exp)
    assert aff(oid, got) == aff(oid, msm.msm(crv, scalars, points))
    srs.close()


@pytest.mark.parametrize("name,n", [("bls12_381_g1", 1 << 14), ("bn254_g1", 1 << 13), ("bn254_g2", 1 << 11), ("bls12_381_g2", 1 << 10)])
def test_srs_prefix_is_the_kzg_call_shape(name, n):
    # kzg.rs:159-163: msm(&coefficients, &srs.powers_main_group[..coefficients.len()])
    from lambda_elliptic_curves_amd import errors, msm
    crv, oid = util.curve_pairs()[name]
    scalars, points = util.msm_case(oid, n, 41)
    srs = msm.Srs(crv, points)
    for m in (n, n - 1, n // 3, 1, 0):
        got = srs.msm(scalars[:m])
        exp = O.parallel_msm_with(oid, scalars[:m], points[:m], max(2, O.optimum_window_size(max(m, 1))), 16) if m else O.ec_neutral(oid)
        assert aff(oid, got) == aff(oid, exp)
    with pytest.raises(errors.LengthMismatch):       # more scalars than points (pippenger.rs:25-27)
        srs.msm(np.concatenate([scalars, scalars[:1]]))
    srs.close()


@pytest.mark.parametrize("name", ["bls12_381_g1", "bn254_g1", "bn254_g2"])
def test_srs_edge_cases(name):
    from lambda_elliptic_curves_amd import msm
    crv, oid = util.curve_pairs()[name]
    g = util.generator(oid)
    neutral = O.ec_neutral(oid)
    r = D.P_FR381 if name == "bls12_381_g1" else D.P_FR254
    p = O.ec_mul(oid, g, 12345, 1)
    # identity rows inside the SRS (first, middle, last), duplicates, P and -P in one bucket, zero scalars, r-1, 2^256-1
    pts = np.stack([neutral, p, p, O.ec_neg(oid, p), neutral, g, g, p, neutral])
    ks = [5, 7, 7, 7, 99, r - 1, 0, (1 << 256) - 1, 3]
    srs = msm.Srs(crv, pts)
    got = srs.msm(O.ints_to_array(ks, 4))
    assert aff(oid, got) == aff(oid, O.msm(oid, O.ints_to_array(ks, 4), pts))
    # a bucket whose first row is the identity, and a sum that cancels to the identity
    pts2 = np.stack([neutral, p, O.ec_neg(oid, p)])
    srs2 = msm.Srs(crv, pts2)
    assert aff(oid, srs2.msm(O.ints_to_array([9, 9, 9], 4))) is None
    # an SRS of identities only, and the empty SRS
    srs3 = msm.Srs(crv, np.stack([neutral, neutral]))
    assert aff(oid, srs3.msm(O.ints_to_array([1, 2], 4))) is None
    srs4 = msm.Srs(crv, np.zeros((0, crv.point_words), np.uint64))
    assert np.array_equal(srs4.msm(np.zeros((0, 4), np.uint64)), neutral)


def test_srs_all_points_equal_and_single_bucket():
    from lambda_elliptic_curves_amd import msm
    crv, oid = util.curve_pairs()["bls12_381_g1"]
    n = 3000
    scalars, points = util.msm_case(oid, n, 6)
    pts = np.tile(points[0], (n, 1))                 # P + P inside every bucket chain (complete formula needed)
    srs = msm.Srs(crv, pts)
    tot = sum(O.array_to_ints(scalars))
    assert aff(oid, srs.msm(scalars)) == aff(oid, O.ec_mul(oid, points[0], tot, 5))
    k = 0x1234567890abcdef1234567890abcdef1234567890abcdef1234567890abcdef
    same = np.tile(O.int_to_limbs(k, 4), (n, 1))     # every point in the same bucket of every window
    srs2 = msm.Srs(crv, points)
    assert aff(oid, srs2.msm(same)) == aff(oid, msm.msm(crv, same, points))


def test_srs_device_resident_large_and_montgomery_scalars():
    # 2^22 points built on the device from a tiled run (the size from which normalisation uses 128-point inversion
    # runs); SRS path == projective path on the same inputs
    import torch
    from lambda_elliptic_curves_amd import msm
    crv, oid = util.curve_pairs()["bls12_381_g1"]
    n, base_n = 1 << 22, 1 << 12
    _, base = util.msm_case(oid, base_n, 77)
    tp = torch.from_numpy(base.view(np.int64)).cuda().repeat(n // base_n, 1)
    rng = np.random.default_rng(78)
    sc = rng.integers(0, 1 << 63, size=(n, 4), dtype=np.uint64)
    ts = torch.from_numpy(sc.view(np.int64)).cuda()
    srs = msm.Srs(crv, t_points=tp, n=n)
    got = srs.msm_device(ts, n)
    assert aff(oid, got) == aff(oid, msm.msm_device(crv, ts, tp, n))
    # FrElements as stored (Montgomery form): representative() on the device, then the SRS MSM
    m = 1 << 10
    vals = [k % D.P_FR381 for k in O.array_to_ints(sc[:m])]
    fr = O.elems_to_mont(O.F_FR381, vals)
    small = msm.Srs(crv, base[:m])
    assert aff(oid, small.msm_fr(fr)) == aff(oid, O.msm(oid, O.ints_to_array(vals, 4), base[:m]))


@pytest.mark.parametrize("name", ["bls12_381_g1", "bn254_g2"])
def test_srs_identity_rows_across_batch_inversion_runs(name):
    # the normalisation inverts z in runs of 32 points; identity rows (z = 0) at the run boundaries must neither
    # poison a run's product nor shift its neighbours
    from lambda_elliptic_curves_amd import msm
    crv, oid = util.curve_pairs()[name]
    n = 100
    scalars, points = util.msm_case(oid, n, 91)
    neutral = O.ec_neutral(oid)
    for i in (0, 31, 32, 33, 63, 64, 95, 96, 99):
        points[i] = neutral
    srs = msm.Srs(crv, points)
    assert aff(oid, srs.msm(scalars)) == aff(oid, O.msm(oid, scalars, points))
    ones = np.zeros((n, 4), np.uint64)
    ones[:, 3] = 1                                   # plain sum of the rows: every normalised row is used as is
    assert aff(oid, srs.msm(ones)) == aff(oid, O.msm(oid, ones, points))
    srs.close()


@pytest.mark.parametrize("name", CURVES)
def test_srs_accumulation_on_one_and_on_four_lanes_per_piece(name, monkeypatch):
    """Small handles accumulate with every addition spread over a quad of lanes (msm_accumulate_quad_kernel<AFFINE>: lanes 0 / 1
    gather x / y, an identity row (0, 0) is recognised across the quad), larger ones with one lane per piece and the mixed
    addition; LW_HIP_MSM_ACCQ (read per call) runs the same handle through both, with identity rows, P / -P, repeated points and
    pieces short enough for several rounds of partial sums."""
    from lambda_elliptic_curves_amd import msm
    crv, oid = util.curve_pairs()[name]
    n = 600
    scalars, points = util.msm_case(oid, n, 4100)
    points = points.copy()
    for i in (0, 1, 77, n - 1):
        points[i] = O.ec_neutral(oid)
    points[11] = points[10]
    points[13] = O.ec_neg(oid, points[12])
    scalars[13] = scalars[12]
    scalars[20:40] = scalars[20]                     # twenty items in the same buckets
    exp = aff(oid, O.msm(oid, scalars, points))
    srs = msm.Srs(crv, points)
    monkeypatch.setenv("LW_HIP_MSM_CH", "4")
    for aq in ("0", "30"):
        monkeypatch.setenv("LW_HIP_MSM_ACCQ", aq)
        assert aff(oid, srs.msm(scalars)) == exp, f"accq = {aq}"
    srs.close()


@pytest.mark.parametrize("name,n", [("bls12_381_g1", 3000), ("bn254_g1", 2000), ("bn254_g2", 700), ("bls12_381_g2", 500)])
def test_folded_srs_matches_oracle_small(name, n, monkeypatch):
    """Large SRS handles keep W = 13 window-shifted copies (row w*n + i = 2^(20 w) P_i) and sort the signed 20-bit digits of
    all windows into ONE set of 2^19 buckets (msm_core.cuh build_fold).  LW_HIP_SRS_FOLD_MIN=0 builds the copies for a small
    set so the whole path — shift kernel, normalisation of the copies (isomorphic model for BN254 G2), shared buckets, prefix
    calls above and below the quarter that switches back to the plain schedule, identity rows, adversarial scalars — meets
    the oracle at a size it finishes instantly."""
    from lambda_elliptic_curves_amd import msm
    crv, oid = util.curve_pairs()[name]
    scalars, points = util.msm_case(oid, n, 1700 + n)
    r = D.P_FR381 if name.startswith("bls") else D.P_FR254
    ks = [int(O.limbs_to_int(row)) for row in scalars]
    for i, v in enumerate([(1 << 256) - 1, 1 << 255, r - 1, 0, 1, (1 << 255) - 1, sum((1 << 19) << (20 * w) for w in range(12)),
                           sum(((1 << 19) + 1) << (20 * w) for w in range(12))]):
        ks[(i * 11) % n] = v
    scalars = O.ints_to_array(ks, 4)
    points = points.copy()
    points[5] = O.ec_neutral(oid)              # identity rows must stay the identity in every shifted copy
    points[n - 1] = O.ec_neutral(oid)
    points[7] = points[6]                      # repeated point
    monkeypatch.setenv("LW_HIP_SRS_FOLD_MIN", "0")
    srs = msm.Srs(crv, points)
    for m in (n, n - 1, n // 2, n // 4 + 1, n // 5, 3, 0):
        got = srs.msm(scalars[:m])
        exp = O.parallel_msm_with(oid, scalars[:m], points[:m], 8, 16) if m else O.ec_neutral(oid)
        assert aff(oid, got) == aff(oid, exp), f"prefix {m}"
    srs.close()


@pytest.mark.parametrize("name,n", [("bls12_381_g1", 4096), ("bn254_g1", 5000)])
def test_folded_srs_single_bucket_holds_every_window(name, n, monkeypatch):
    """A folded SRS sorts the items of ALL windows into one bucket set, so a bucket can hold n * W items, not n: every scalar
    with the same digit in every window (sum_w 2^(20 w): bucket 0 receives 13 n items; 2^20 + 1: two windows' worth) needs
    more rounds of partial sums than a plain MSM of n points — the workspace is sized for that (msm_core.cuh run)."""
    from lambda_elliptic_curves_amd import msm
    crv, oid = util.curve_pairs()[name]
    _, points = util.msm_case(oid, n, 4100 + n)
    monkeypatch.setenv("LW_HIP_SRS_FOLD_MIN", "0")
    srs = msm.Srs(crv, points)
    for k in (sum(1 << (20 * w) for w in range(13)), (1 << 20) + 1, sum((1 << 19) << (20 * w) for w in range(12))):
        scalars = O.ints_to_array([k] * n, 4)
        exp = O.parallel_msm_with(oid, scalars, points, 8, 16)
        assert aff(oid, srs.msm(scalars)) == aff(oid, exp), hex(k)
    srs.close()


def test_fold_is_per_call(monkeypatch):
    """Whether a call runs on the shifted copies is decided per call and handed down as an argument: a folded call, a prefix
    below the quarter (plain schedule on copy 0), a folded call again and a plain msm() of the same points on the same lane,
    each against the oracle — nothing of one call's fold may reach the next."""
    from lambda_elliptic_curves_amd import msm
    crv, oid = util.curve_pairs()["bls12_381_g1"]
    n = 3000
    scalars, points = util.msm_case(oid, n, 5150)
    exp = {m: aff(oid, O.parallel_msm_with(oid, scalars[:m], points[:m], 8, 16)) for m in (n, n // 5)}
    monkeypatch.setenv("LW_HIP_SRS_FOLD_MIN", "0")
    srs = msm.Srs(crv, points)
    for m in (n, n // 5, n):
        assert aff(oid, srs.msm(scalars[:m])) == exp[m], f"prefix {m}"
    assert aff(oid, msm.msm(crv, scalars, points)) == exp[n]
    srs.close()


def test_folded_srs_matches_oracle_at_default_threshold():
    """2^19 points: the smallest set that is folded by default (BLS12-381 G1), against the oracle."""
    from lambda_elliptic_curves_amd import msm
    crv, oid = util.curve_pairs()["bls12_381_g1"]
    n = 1 << 19
    scalars, points = util.msm_case(oid, n, 2024, threads=util.host_threads())
    srs = msm.Srs(crv, points)
    exp = aff(oid, O.parallel_msm_with(oid, scalars, points, 15, util.host_threads()))
    assert aff(oid, srs.msm(scalars)) == exp
    srs.close()
