"""Multilinear evaluate / fix_variables and the sumcheck round on the device (lw_multilinear_*, lw_sumcheck_round*)
against tests/multilinear_ref.py, bit for bit in the stored (Montgomery) form, on Stark252 and BLS12-381 Fr.

The kernels' schedule (lambda_elliptic_curves_amd/csrc/multilinear.hip) and the sizes that cross its boundaries:
  evaluate   a block folds the last 11 variables of a run of 2^11 elements: thread r takes the elements r + 256 e, e < 8,
             and the eq weights come from three small tables over index bits 0..3, 4..7 and 8..10.  So n = 4 | 5 and 8 | 9
             start a new table, n = 8 | 9 is also one | several elements per thread, n = 11 | 12 is one | two blocks and the
             first call with a second launch over the block sums; 2^18 gives that launch 128 sums per table.  Tables go on
             blockIdx.y eight at a time: K = 9 is a second group.
  fix        at most 3 variables per pass: t = 4 is two passes (first workspace buffer), t = 7 three (both buffers);
             256 results per block: 2^(n-t) = 256 | 512.
  round      256 pairs per block and at most 1024 blocks: q = 2^(n-1) (plain) or 2^(n-2) (fused) pairs, so n = 9 | 10
             (fused 10 | 11) is one | two blocks, and above 2^18 pairs a thread takes a second pair: plain at n = 20."""
import functools
import hashlib

import numpy as np
import pytest

from tests import multilinear_ref as M
from tests.util import dev, fld, host, rand_elems, to_arr, to_ints

pytestmark = pytest.mark.gpu
FIELDS = ["stark252", "fr381"]
F_REF = {name: M.Fld(M.MODULI[name], True) for name in FIELDS}


@functools.lru_cache(maxsize=None)
def case(name, n, k, seed=0):
    """k tables of 2^n elements and a point, as arrays and as integers; computed once, never modified"""
    arrs = [rand_elems(name, 1 << n, 1000 * n + 10 * i + seed) for i in range(k)]
    pt = rand_elems(name, max(n, 1), 77 + n + seed)[:n]
    return arrs, [to_ints(a) for a in arrs], pt, to_ints(pt)


@functools.lru_cache(maxsize=None)
def bound_case(name, n, seed=0):
    """the three tables of case(name, n, 3) bound to a challenge: (r array, r, bound tables as integers)"""
    _, ints, _, _ = case(name, n, 3, seed)
    r = rand_elems(name, 1, 5 + n + seed)
    return r[0], to_ints(r)[0], [M.fix_variables(F_REF[name], T, [to_ints(r)[0]]) for T in ints]


@pytest.mark.parametrize("name", FIELDS)
def test_evaluate_matches_reference(name):
    from lambda_elliptic_curves_amd import multilinear
    F, R = fld(name), F_REF[name]
    for n in range(0, 15):
        arrs, ints, pt, pti = case(name, n, 3)
        want = [M.evaluate(R, T, pti) for T in ints]
        assert to_ints(multilinear.evaluate(F, arrs[:1], pt)) == want[:1], n
        assert to_ints(multilinear.evaluate(F, arrs, pt)) == want, n
        ts = [dev(a) for a in arrs]
        assert to_ints(multilinear.evaluate_device(F, ts[:1], n, pt)) == want[:1], n
        assert to_ints(multilinear.evaluate_device(F, ts, n, pt)) == want, n
    for n in (3, 12):   # nine tables: a second group on blockIdx.y
        arrs, ints, pt, pti = case(name, n, 3)
        order = [0, 1, 2, 2, 1, 0, 1, 0, 2]
        got = multilinear.evaluate(F, [arrs[i] for i in order], pt)
        assert to_ints(got) == [M.evaluate(R, ints[i], pti) for i in order]


@pytest.mark.parametrize("name", FIELDS)
def test_fix_variables_matches_reference(name):
    import torch
    from lambda_elliptic_curves_amd import multilinear
    F, R = fld(name), F_REF[name]
    for n in range(0, 15):
        arrs, ints, pt, pti = case(name, n, 3)
        t_tab = dev(arrs[0])
        for t in sorted({0, 1, 2, 3, 4, 7, n}):
            if t > n:
                continue
            want = M.fix_variables(R, ints[0], pti[:t])
            assert to_ints(multilinear.fix_variables(F, arrs[0], pt[:t])) == want, (n, t)
            t_out = torch.zeros((1 << (n - t), 4), dtype=torch.int64, device="cuda")
            multilinear.fix_variables_device(F, t_tab, n, pt[:t], t_out)
            torch.cuda.synchronize()
            assert to_ints(host(t_out)) == want, (n, t)
        assert np.array_equal(host(t_tab), arrs[0])   # the table is only read


@pytest.mark.parametrize("name", FIELDS)
def test_evaluate_and_fix_variables_2_18(name):
    import torch
    from lambda_elliptic_curves_amd import multilinear
    F, R, n = fld(name), F_REF[name], 18
    arrs, ints, pt, pti = case(name, n, 3)
    ts = [dev(a) for a in arrs]
    w = M.chis(R, pti)
    want = [sum(R.mul(a, b) for a, b in zip(T, w)) % R.p for T in ints]
    assert to_ints(multilinear.evaluate_device(F, ts, n, pt)) == want
    assert to_ints(multilinear.evaluate_device(F, ts[1:2], n, pt)) == want[1:2]
    assert to_ints(multilinear.evaluate(F, arrs[2:], pt)) == want[2:]
    for t in (1, 4, n):
        t_out = torch.zeros((1 << (n - t), 4), dtype=torch.int64, device="cuda")
        multilinear.fix_variables_device(F, ts[0], n, pt[:t], t_out)
        torch.cuda.synchronize()
        assert to_ints(host(t_out)) == M.fix_variables(R, ints[0], pti[:t]), t
    assert to_ints(host(t_out)) == want[:1]   # t = n is evaluate


@pytest.mark.parametrize("name", FIELDS)
def test_operand_edges(name):
    import torch
    from lambda_elliptic_curves_amd import multilinear
    F, R = fld(name), F_REF[name]
    p = R.p
    ones = ((1 << 256) - 1) % p   # limbs of all ones, reduced
    for n in (3, 12):
        N = 1 << n
        rnd = case(name, n, 3)[1][0]
        tables = {"p - 1": [p - 1] * N, "all ones": [ones] * N, "zeros": [0] * N, "random": rnd}
        points = {"p - 1": [p - 1] * n, "all ones": [ones] * n, "zero": [0] * n, "one": [R.one] * n,
                  "bits": [R.one if (0x5a3 >> j) & 1 else 0 for j in range(n)]}
        for tn, T in tables.items():
            for pn, r in points.items():
                tag = (n, tn, pn)
                want = M.evaluate(R, T, r)
                if pn in ("zero", "one", "bits"):   # r_j in {0, 1} selects one entry exactly
                    idx = int("".join("1" if v else "0" for v in r), 2)
                    assert want == T[idx]
                if tn == "zeros":
                    assert want == 0
                assert to_ints(multilinear.evaluate(F, [to_arr(T)], to_arr(r))) == [want], tag
                for t in (2, 5):
                    if t > n:
                        continue
                    got = to_ints(multilinear.fix_variables(F, to_arr(T), to_arr(r[:t])))
                    assert got == M.fix_variables(R, T, r[:t]), tag + (t,)
                    if pn in ("zero", "one", "bits"):   # ... or one 2^(n-t)-th of the table
                        b = int("".join("1" if v else "0" for v in r[:t]), 2)
                        assert got == T[b << (n - t):(b + 1) << (n - t)], tag + (t,)
                # a round over (T, T, random) bound to r[0]
                tabs = [T, T, rnd]
                assert to_ints(multilinear.sumcheck_round(F, [to_arr(x) for x in tabs])) == M.round_poly(R, tabs), tag
                ts = [dev(to_arr(x)) for x in tabs]
                bound = [M.fix_variables(R, x, r[:1]) for x in tabs]
                g = multilinear.sumcheck_round_device(F, ts, n, to_arr(r[:1])[0])
                assert to_ints(g) == M.round_poly(R, bound), tag
                assert [to_ints(host(x)[:N // 2]) for x in ts] == bound, tag


def _check_rounds(name, n, K, seed=0):
    import torch
    from lambda_elliptic_curves_amd import multilinear
    F, R = fld(name), F_REF[name]
    arrs, ints, _, _ = case(name, n, 3, seed)
    arrs, ints = arrs[:K], ints[:K]
    ts = [dev(a) for a in arrs]
    want = M.round_poly(R, ints)
    assert to_ints(multilinear.sumcheck_round_device(F, ts, n)) == want, (n, K)
    assert all(np.array_equal(host(t), a) for t, a in zip(ts, arrs))   # a plain round only reads
    if n < 2:
        return
    r_arr, r, bound = bound_case(name, n, seed)
    want_f = M.round_poly(R, bound[:K])
    h = 1 << (n - 1)
    g = multilinear.sumcheck_round_device(F, ts, n, r_arr)
    assert to_ints(g) == want_f, (n, K)
    for t, b in zip(ts, bound):
        assert to_ints(host(t)[:h]) == b, (n, K)
    if n <= 12:   # the host form: the same values, the bound tables written back to the first halves
        hs = [a.copy() for a in arrs]
        assert to_ints(multilinear.sumcheck_round(F, hs)) == want
        assert to_ints(multilinear.sumcheck_round(F, hs, r_arr)) == want_f
        for a, b in zip(hs, bound):
            assert to_ints(a[:h]) == b


@pytest.mark.parametrize("name", FIELDS)
@pytest.mark.parametrize("K", [1, 2, 3])
def test_sumcheck_round_matches_reference(name, K):
    for n in range(1, 15):
        _check_rounds(name, n, K)


@pytest.mark.parametrize("name", FIELDS)
@pytest.mark.parametrize("K", [1, 2, 3])
def test_sumcheck_round_2_18(name, K):
    _check_rounds(name, 18, K)


@pytest.mark.parametrize("name", FIELDS)
def test_sumcheck_round_plain_2_20_second_pair_per_thread(name):
    from lambda_elliptic_curves_amd import multilinear
    R, n = F_REF[name], 20
    arr = rand_elems(name, 1 << n, 3)
    T = to_ints(arr)
    h = 1 << (n - 1)
    want = [sum(T[:h]) % R.p, sum(T[h:]) % R.p]   # K = 1: g(0) and g(1) are the sums of the halves
    assert to_ints(multilinear.sumcheck_round_device(fld(name), [dev(arr)], n)) == want


def _sha3_challenge(p):
    def ch(g):
        g = np.ascontiguousarray(g, dtype=np.uint64)
        return to_arr([int.from_bytes(hashlib.sha3_256(g.astype(">u8").tobytes()).digest(), "big") % p])[0]
    return ch


@pytest.mark.parametrize("name", FIELDS)
@pytest.mark.parametrize("n", [1, 2, 11])
def test_sumcheck_prove_device(name, n):
    from lambda_elliptic_curves_amd import multilinear
    F, R = fld(name), F_REF[name]
    arrs, ints, _, _ = case(name, n, 3, seed=1)
    ch = _sha3_challenge(R.p)
    claimed, rounds, point, final = multilinear.sumcheck_prove_device(F, [dev(a) for a in arrs], n, ch)
    claimed, rounds, point, final = to_ints(claimed)[0], [to_ints(g) for g in rounds], to_ints(point), to_ints(final)
    assert len(rounds) == n and len(point) == n and len(final) == 3
    assert claimed == M.cube_sum(R, ints)
    assert M.verify(R, claimed, rounds, point, final)
    # the same transcript as the honest Python prover, value for value
    assert (claimed, rounds, point, final) == M.prove(R, ints, lambda g: to_ints(ch(to_arr(g)))[0])
    assert final == [M.evaluate(R, T, point) for T in ints]


@pytest.mark.parametrize("name", FIELDS)
def test_side_stream(name):
    import torch
    from lambda_elliptic_curves_amd import multilinear
    F, R, n = fld(name), F_REF[name], 13
    arrs, ints, pt, pti = case(name, n, 3)
    r_arr, r, bound = bound_case(name, n)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        ts = [dev(a) for a in arrs]
        t_out = torch.zeros((1 << (n - 4), 4), dtype=torch.int64, device="cuda")
        s.synchronize()
        ev = multilinear.evaluate_device(F, ts, n, pt, stream=s.cuda_stream)
        multilinear.fix_variables_device(F, ts[0], n, pt[:4], t_out, stream=s.cuda_stream)
        g = multilinear.sumcheck_round_device(F, ts, n, r_arr, stream=s.cuda_stream)   # synchronises: t_out is complete too
    assert to_ints(ev) == [M.evaluate(R, T, pti) for T in ints]
    assert to_ints(host(t_out)) == M.fix_variables(R, ints[0], pti[:4])
    assert to_ints(g) == M.round_poly(R, bound)
