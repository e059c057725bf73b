"""GPU parity: HIP NTT (through the C ABI) vs the CPU oracle, bit-exact on raw Montgomery limbs.
Mirrors the reference's GPU-vs-CPU tests (math/src/fft/gpu/cuda/ops.rs:109-136: proptest sizes + the 2^20
all-ones vector) and the Polynomial API property tests (math/src/fft/polynomial.rs:302-457)."""
import numpy as np
import pytest

from oracle import oracle as O
from tests import util

pytestmark = pytest.mark.gpu

F256 = ["stark252", "fr381"]


def _pair(name):
    return util.field_pairs()[name]


@pytest.mark.parametrize("name", F256)
@pytest.mark.parametrize("log_n", list(range(0, 15)))
def test_evaluate_fft_matches_oracle_all_small_sizes(name, log_n):
    from lambda_elliptic_curves_amd import fft
    fld, oid = _pair(name)
    a = util.rand_elems(name, 1 << log_n, 1000 + log_n)
    a[-1, -1] |= np.uint64(1)          # keep the leading coefficient non-zero (Polynomial::new strips zeros)
    got = fft.evaluate_fft(fld, a)
    exp = O.evaluate_fft(oid, a)
    assert got.shape == exp.shape and np.array_equal(got, exp)


@pytest.mark.parametrize("name", F256)
@pytest.mark.parametrize("log_n", [1, 2, 3, 5, 8, 9, 11, 12, 13, 16])
def test_interpolate_fft_matches_oracle_and_roundtrips(name, log_n):
    from lambda_elliptic_curves_amd import fft
    fld, oid = _pair(name)
    a = util.rand_elems(name, 1 << log_n, 2000 + log_n)
    got = fft.interpolate_fft(fld, a)
    assert np.array_equal(got, O.interpolate_fft(oid, a))
    assert np.array_equal(fft.evaluate_fft(fld, got, 1, 1 << log_n), a) or log_n == 0


@pytest.mark.parametrize("name", F256)
@pytest.mark.parametrize("log_n,h", [(3, 3), (6, 7), (10, 3), (13, 2), (17, 7), (20, 5), (22, 3)])   # 2^20, 2^22: 6- and 7-stage passes with the coset factor (compiled-in tile shapes)
def test_offset_variants(name, log_n, h):
    from lambda_elliptic_curves_amd import fft
    fld, oid = _pair(name)
    a = util.rand_elems(name, 1 << log_n, 3000 + log_n)
    a[-1, -1] |= np.uint64(1)
    off = util.offset_elem(name, h)
    ev = fft.evaluate_offset_fft(fld, a, 1, None, off)
    assert np.array_equal(ev, O.evaluate_fft(oid, a, 1, None, off))
    back = fft.interpolate_offset_fft(fld, ev, off)
    assert np.array_equal(back, O.interpolate_fft(oid, ev, off))
    assert np.array_equal(back, a)


@pytest.mark.parametrize("name", F256)
def test_length_rule_padding_and_zero_poly(name):
    from lambda_elliptic_curves_amd import fft
    fld, oid = _pair(name)
    for ncoef, blowup, ds in [(5, 1, None), (8, 2, None), (3, 4, 16), (1, 1, None), (7, 1, 4), (6, 8, None), (100, 2, 64)]:
        a = util.rand_elems(name, ncoef, 42 + ncoef)
        a[-1, -1] |= np.uint64(1)
        got = fft.evaluate_fft(fld, a, blowup, ds)
        exp = O.evaluate_fft(oid, a, blowup, ds)
        assert got.shape == exp.shape and np.array_equal(got, exp)
    # trailing zero coefficients are stripped before the length rule
    a = util.rand_elems(name, 4, 5)
    a[2:] = 0
    assert fft.evaluate_fft(fld, a).shape[0] == 2
    z = fft.evaluate_fft(fld, np.zeros((3, 4), np.uint64), 2, 8)
    assert z.shape[0] == 16 and not z.any()
    # interpolate strips trailing zeros of the result (constant polynomial)
    ev = fft.evaluate_fft(fld, util.rand_elems(name, 1, 9) | np.uint64(1), 1, 8)
    assert fft.interpolate_fft(fld, ev, strip=True).shape[0] == 1


@pytest.mark.parametrize("name", F256)
def test_errors_mirror_reference(name):
    from lambda_elliptic_curves_amd import errors, fft
    fld, oid = _pair(name)
    with pytest.raises(errors.InputError):       # ops::fft: InputError for non power of two
        fft.interpolate_fft(fld, util.rand_elems(name, 3, 1))
    with pytest.raises(errors.InputError):       # blowup 3 makes len non power of two
        fft.evaluate_fft(fld, util.rand_elems(name, 4, 1) | np.uint64(1), 3)
    if name == "fr381":                          # TWO_ADICITY 32: order 33 has no root of unity
        with pytest.raises(errors.RootOfUnityError):
            fft.ntt(fld, util.rand_elems(name, 2, 1), log2n=33)
    with pytest.raises(errors.OrderError):
        fft.ntt(fld, util.rand_elems(name, 2, 1), log2n=64)


def test_stark252_all_ones_2_20():
    # the reference's own large GPU test vector (math/src/fft/gpu/cuda/ops.rs:124-136)
    from lambda_elliptic_curves_amd import fft
    fld, oid = _pair("stark252")
    one = O.field_params(oid)["one"]
    a = np.tile(O.int_to_limbs(one, 4), (1 << 20, 1))
    got = fft.ntt(fld, a)
    tw = O.get_twiddles(oid, 20, O.ROOTS_BITREV)
    assert np.array_equal(got, O.fft(oid, a, tw))


@pytest.mark.parametrize("name", F256)
def test_random_2_20_forward_inverse(name):
    from lambda_elliptic_curves_amd import fft
    fld, oid = _pair(name)
    a = util.rand_elems(name, 1 << 20, 77)
    got = fft.ntt(fld, a)
    assert np.array_equal(got, O.fft(oid, a, O.get_twiddles(oid, 20, O.ROOTS_BITREV)))
    assert np.array_equal(fft.ntt(fld, got, inverse=True), a)


@pytest.mark.parametrize("name", F256)
def test_batched_strided_and_in_place(name):
    from lambda_elliptic_curves_amd import fft
    fld, oid = _pair(name)
    log_n, batch, stride = 10, 5, 1024 + 64
    buf = util.rand_elems(name, batch * stride, 11)
    got = fft.ntt(fld, buf, log2n=log_n, batch=batch, batch_stride=stride)
    tw = O.get_twiddles(oid, log_n, O.ROOTS_BITREV)
    for b in range(batch):
        seg = buf[b * stride:b * stride + 1024]
        assert np.array_equal(got[b * stride:b * stride + 1024], O.fft(oid, seg, tw))


def test_device_resident_matches_host_path_and_large_roundtrip():
    import torch
    from lambda_elliptic_curves_amd import fft
    fld, oid = _pair("stark252")
    for log_n in (12, 22):
        a = util.rand_elems("stark252", 1 << log_n, 5 + log_n)
        t_in = torch.from_numpy(a.view(np.int64)).cuda()
        t_out = torch.empty_like(t_in)
        fft.ntt_device(fld, t_in, t_out, log_n)
        torch.cuda.synchronize()
        ev = t_out.cpu().numpy().view(np.uint64)
        if log_n == 12:
            assert np.array_equal(ev, O.evaluate_fft(oid, a))
        # in-place inverse on the device buffer restores the input (size-independent property)
        fft.ntt_device(fld, t_out, t_out, log_n, inverse=True)
        torch.cuda.synchronize()
        assert np.array_equal(t_out.cpu().numpy().view(np.uint64), a)
        # linearity spot check: NTT(a)[0] = sum(a)  <=> inverse of constant... (checked via oracle at 2^12 only)


@pytest.mark.parametrize("name", ["stark252", "fr381", "babybear_u32", "babybear_u64"])
def test_gen_twiddles_and_bitrev_permutation_match_oracle(name):
    # the other two ops of the reference's GPU seam (math/src/fft/gpu/cuda/ops.rs:45-77; fuzz twiddles_generation_diff)
    from lambda_elliptic_curves_amd import errors, fft
    fld, oid = util.field_pairs()[name]
    for order in (0, 1, 2, 5, 11, 17):
        for cfg, ocfg in ((fft.ROOTS_NATURAL, O.ROOTS_NATURAL), (fft.ROOTS_NATURAL_INVERSED, O.ROOTS_NATURAL_INV),
                          (fft.ROOTS_BIT_REVERSE, O.ROOTS_BITREV), (fft.ROOTS_BIT_REVERSE_INVERSED, O.ROOTS_BITREV_INV)):
            got = fft.get_twiddles(fld, order, cfg)
            exp = O.get_twiddles(oid, order, ocfg)
            assert got.size == exp.size and np.array_equal(got.reshape(-1), exp.reshape(-1))
    with pytest.raises(errors.OrderError):     # roots_of_unity.rs:70-72
        fft.get_twiddles(fld, 64, fft.ROOTS_NATURAL)
    for log_n in (0, 1, 4, 13):
        a = util.rand_elems(name, 1 << log_n, 31 + log_n)
        got = fft.bitrev_permutation(fld, a)
        assert np.array_equal(got.reshape(-1), O.bit_reverse_permute(oid, a).reshape(-1))
    with pytest.raises(errors.InputError):
        fft.bitrev_permutation(fld, util.rand_elems(name, 3, 1))


@pytest.mark.parametrize("name", F256)
@pytest.mark.parametrize("log_m,blow", [(0, 2), (1, 1), (3, 2), (6, 3), (9, 3), (12, 1), (13, 4), (16, 3), (17, 1)])
def test_low_degree_extension_path(name, log_m, blow):
    # evaluate_offset_fft(poly, blowup, Some(n), offset) as the STARK prover calls it (provers/stark/src/prover.rs:150-167);
    # the device skips the stages that only replicate the zero-padded block — bytes must not change
    import torch
    from lambda_elliptic_curves_amd import fft
    fld, oid = _pair(name)
    n = 1 << log_m
    a = util.rand_elems(name, n, 600 + log_m)
    a[-1, -1] |= np.uint64(1)
    off = util.offset_elem(name, 3)
    exp = O.evaluate_fft(oid, a, 1 << blow, n, off)
    assert np.array_equal(fft.evaluate_offset_fft(fld, a, 1 << blow, n, off), exp)
    assert np.array_equal(fft.evaluate_fft(fld, a, 1 << blow, n), O.evaluate_fft(oid, a, 1 << blow, n))
    # fewer coefficients than the block (degree < n - 1) and the device entry point with a batch of 2
    short = a[: max(1, n - n // 3)].copy()
    short[-1, -1] |= np.uint64(1)
    assert np.array_equal(fft.evaluate_offset_fft(fld, short, 1 << blow, n, off), O.evaluate_fft(oid, short, 1 << blow, n, off))
    two = np.concatenate([a, util.rand_elems(name, n, 5)])
    t_in = torch.from_numpy(two.view(np.int64)).cuda()
    t_out = torch.empty((2 << (log_m + blow), 4), dtype=torch.int64, device="cuda")
    fft.lde_device(fld, t_in, log_m, t_out, log_m + blow, batch=2, offset=off)
    torch.cuda.synchronize()
    got = t_out.cpu().numpy().view(np.uint64)
    N = n << blow
    assert np.array_equal(got[:N], exp)
    pad = np.zeros((N, 4), np.uint64); pad[:n] = two[n:]
    assert np.array_equal(got[N:], O.evaluate_fft(oid, pad, 1, N, off))


def test_full_size_2_26_round_trip_and_dc_term():
    # BASELINE configs[1] upper end: 2^26 Stark252 elements (2 GiB per buffer), device-resident.  Size-independent
    # properties: INTT(NTT(x)) == x, and output 0 is the sum of the inputs (raw Montgomery values add linearly).
    import torch
    from lambda_elliptic_curves_amd import fft
    fld, oid = _pair("stark252")
    L = 26
    p = 0x800000000000011000000000000000000000000000000000000000000000001
    a = util.rand_elems("stark252", 1 << L, 2026)
    total = 0
    for k in range(4):                       # limb k has weight 2^(64*(3-k)); split in halves to avoid overflow
        col = a[:, k]
        total += (int(np.sum(col >> np.uint64(32), dtype=np.uint64)) << 32) + int(np.sum(col & np.uint64(0xffffffff), dtype=np.uint64)) << (64 * (3 - k))
    t_in = torch.from_numpy(a.view(np.int64)).cuda()
    t_out = torch.empty_like(t_in)
    fft.ntt_device(fld, t_in, t_out, L)
    torch.cuda.synchronize()
    first = t_out[:1].cpu().numpy().view(np.uint64)
    assert O.limbs_to_int(first[0]) == total % p
    fft.ntt_device(fld, t_out, t_out, L, inverse=True)
    torch.cuda.synchronize()
    assert torch.equal(t_out, t_in)


@pytest.mark.parametrize("name", ["stark252", "fr381", "babybear_u32", "babybear_u64"])
def test_get_powers_of_primitive_root_and_coset_variant(name):
    # roots_of_unity.rs:13-61: arbitrary `count` (also past the group order), all four configurations, and the coset
    # variant offset * w^i; the bit-reversed configurations return next_power_of_two(count) entries
    from lambda_elliptic_curves_amd import errors, fft
    from oracle import bigint_def as D
    fld, oid = util.field_pairs()[name]
    tw_oid = oid
    for n, count in ((4, 16), (4, 40), (10, 1000), (12, 5), (0, 3), (3, 1)):
        for cfg, ocfg in ((fft.ROOTS_NATURAL, O.ROOTS_NATURAL), (fft.ROOTS_NATURAL_INVERSED, O.ROOTS_NATURAL_INV),
                          (fft.ROOTS_BIT_REVERSE, O.ROOTS_BITREV), (fft.ROOTS_BIT_REVERSE_INVERSED, O.ROOTS_BITREV_INV)):
            got = fft.get_powers_of_primitive_root(fld, n, count, cfg)
            exp = O.get_powers_of_primitive_root(tw_oid, n, count, ocfg)
            assert got.size == exp.size and np.array_equal(got.reshape(-1), np.asarray(exp).reshape(-1)), (n, count, cfg)
    assert fft.get_powers_of_primitive_root(fld, 5, 0, fft.ROOTS_NATURAL).size == 0
    p = {"stark252": D.P_STARK252, "fr381": D.P_FR381}.get(name, D.P_BABYBEAR)
    n, count, h = 9, 777, 7
    w = D.primitive_root_of_unity(p, n)
    exp = O.elems_to_mont(oid, [h * pow(w, i, p) % p for i in range(count)])
    got = fft.get_powers_of_primitive_root_coset(fld, n, count, util.offset_elem(name, h))
    assert np.array_equal(got.reshape(-1), np.asarray(exp).reshape(-1))
    with pytest.raises(errors.RootOfUnityError):
        fft.get_powers_of_primitive_root(fld, fld.two_adicity + 1, 4, fft.ROOTS_NATURAL)


@pytest.mark.parametrize("name", F256)
@pytest.mark.parametrize("in_place", [False, True])
@pytest.mark.parametrize("inverse", [False, True])
def test_batch_split_above_32768_columns(name, inverse, in_place):
    util.check_ntt_split(name, inverse, in_place)


@pytest.mark.parametrize("name", F256)
def test_lde_batch_split_above_32768_blocks(name):
    util.check_ntt_lde_split(name)


@pytest.mark.parametrize("name", F256)
@pytest.mark.parametrize("log_n", [1, 5, 8, 9])
def test_strided_columns_with_canaries_distinct_and_in_place(name, log_n):
    util.check_ntt_strided(name, log_n)
