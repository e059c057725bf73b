"""The eq table and the sumcheck round over an eq-weighted sum of products on the device (lw_multilinear_eq_table*,
lw_sumcheck_terms_round*) against tests/sumcheck_terms_ref.py and tests/multilinear_ref.py, bit for bit in the stored
(Montgomery) form, on Stark252 and BLS12-381 Fr.

The kernels' schedule (lambda_elliptic_curves_amd/csrc/sumcheck_terms.hip) and the sizes that cross its boundaries:
  eq table   two half tables over the leading n - n/2 and the trailing n/2 variables, then one product per element: n = 0 and
             n = 1 have a half table of one element, odd and even n split differently, 256 elements per block: n = 8 | 9.
  round      as the product round: 256 pairs per block and at most 1024 blocks, q = 2^(n-1) (plain) or 2^(n-2) (fused) pairs,
             so n = 9 | 10 (fused 10 | 11) is one | two blocks, and above 2^18 pairs a thread takes a second pair: plain at
             n = 20, fused at n = 21.  One kernel per number of tables M = 1 .. 4, with and without eq, plain and fused.
The term lists are those of sumcheck_terms_ref.term_lists.  A single term over all tables stops at three tables when
M = 4, since a term takes at most three.  All term lists run at n = 1 .. 14; at n = 18, where the Python restatement
costs seconds, every M with and without eq runs one list: A B - C from three tables on, the single term below."""
import functools
import hashlib

import numpy as np
import pytest

from tests import multilinear_ref as M
from tests import sumcheck_terms_ref as T
from tests.util import dev, fld, host, rand_elems, to_arr, to_ints

pytestmark = pytest.mark.gpu
FIELDS = ["stark252", "fr381"]
F_REF = {name: M.Fld(M.MODULI[name], True) for name in FIELDS}
TAGS = {1: ["all", "eight"], 2: ["all", "eight"], 3: ["A B - C", "all", "eight"],
        4: ["A B - C", "rA A D + rB B D + rC C D", "A B C + D", "all", "eight"]}
SHAPES = [(m, has_eq, tag) for m in (1, 2, 3, 4) for has_eq in (False, True) for tag in TAGS[m]]


def limb_sum(a):
    """the sum of the elements of a (N, 4) uint64 array, N <= 2^20, as a Python integer"""
    total = 0
    for k in range(4):
        col = a[:, k]
        lo, hi = int((col & np.uint64(0xffffffff)).sum(dtype=np.uint64)), int((col >> np.uint64(32)).sum(dtype=np.uint64))
        total += (lo + (hi << 32)) << (64 * (3 - k))
    return total


@functools.lru_cache(maxsize=None)
def case(name, n):
    """five tables of 2^n elements (A, B, C, D and a random table for the eq slot), as arrays and as integers; computed
    once, never modified"""
    arrs = [rand_elems(name, 1 << n, 2000 * n + 10 * i) for i in range(5)]
    return arrs, [to_ints(a) for a in arrs]


@functools.lru_cache(maxsize=None)
def bound_case(name, n):
    """the five tables of case(name, n) bound to a challenge: (r array, bound tables as integers)"""
    r = rand_elems(name, 1, 9 + n)
    return r[0], [M.fix_variables(F_REF[name], X, [to_ints(r)[0]]) for X in case(name, n)[1]]


@functools.lru_cache(maxsize=None)
def coeffs(name):
    return to_ints(rand_elems(name, 3, 4242))


def py_terms(terms):
    """integer coefficients -> the (4,) arrays the library takes"""
    return [(None if c is None else to_arr([c])[0], idx) for c, idx in terms]


# ---- eq table ----
@pytest.mark.parametrize("name", FIELDS)
def test_eq_table_matches_chis(name):
    import torch
    from lambda_elliptic_curves_amd import multilinear
    F, R = fld(name), F_REF[name]
    for n in list(range(0, 15)) + [18]:
        pt = rand_elems(name, max(n, 1), 300 + n)[:n]
        want = M.chis(R, to_ints(pt))
        t = multilinear.eq_table_device(F, pt)
        torch.cuda.synchronize()
        assert to_ints(host(t)) == want, n
        if n <= 12:
            assert to_ints(multilinear.eq_table(F, pt)) == want, n
    # into a tensor of the caller's, larger than the table: the rest is not touched
    t_out = torch.full((64, 4), -1, dtype=torch.int64, device="cuda")
    pt = rand_elems(name, 5, 305)
    assert multilinear.eq_table_device(F, pt, t_out) is t_out
    torch.cuda.synchronize()
    assert to_ints(host(t_out)[:32]) == M.chis(R, to_ints(pt)) and bool((t_out[32:] == -1).all())


@pytest.mark.parametrize("name", FIELDS)
def test_eq_table_of_a_cube_point_selects_one_index_2_22(name):
    import torch
    from lambda_elliptic_curves_amd import multilinear
    F, R, n = fld(name), F_REF[name], 22
    bits = [(0x2b5a93 >> j) & 1 for j in range(n)]
    idx = int("".join(str(b) for b in bits), 2)   # coordinate 0 is the most significant bit of the index
    t = multilinear.eq_table_device(F, to_arr([R.one if b else 0 for b in bits]))
    torch.cuda.synchronize()
    is_one = (t == dev(to_arr([R.one]))).all(dim=1)
    assert int(is_one.sum()) == 1 and int(is_one.nonzero()[0, 0]) == idx
    assert int((t != 0).any(dim=1).sum()) == 1


@pytest.mark.parametrize("name", FIELDS)
def test_eq_table_evaluates_to_eq_2_22(name):
    from lambda_elliptic_curves_amd import multilinear
    F, R, n = fld(name), F_REF[name], 22
    r, s = rand_elems(name, n, 31), rand_elems(name, n, 32)
    t = multilinear.eq_table_device(F, r)
    assert to_ints(multilinear.evaluate_device(F, [t], n, s)) == [T.eq_closed_form(R, to_ints(r), to_ints(s))]


@pytest.mark.parametrize("name", FIELDS)
def test_eq_table_coordinate_edges(name):
    import torch
    from lambda_elliptic_curves_amd import multilinear
    F, R = fld(name), F_REF[name]
    p = R.p
    ones = ((1 << 256) - 1) % p   # limbs of all ones, reduced
    rnd = to_ints(rand_elems(name, 13, 33))
    for n in (1, 5, 13):
        points = {"p - 1": [p - 1] * n, "all ones": [ones] * n, "zero": [0] * n, "one": [R.one] * n, "minus one": [p - R.one] * n,
                  "mixed": [(p - 1, ones, 0, R.one, rnd[j])[j % 5] for j in range(n)]}
        for pn, r in points.items():
            t = multilinear.eq_table_device(F, to_arr(r))
            torch.cuda.synchronize()
            assert to_ints(host(t)) == M.chis(R, r), (n, pn)


# ---- round ----
def _check_round(name, n, m, has_eq, terms, host_form):
    from lambda_elliptic_curves_amd import multilinear
    F, R = fld(name), F_REF[name]
    arrs, ints = case(name, n)
    sel = list(range(m)) + ([4] if has_eq else [])
    pt = py_terms(terms)
    D = T.degree(terms, has_eq)
    ts = [dev(arrs[i]) for i in sel]
    te = ts[m] if has_eq else None
    want = T.round_poly(R, [ints[i] for i in range(m)], terms, ints[4] if has_eq else None)
    g = multilinear.sumcheck_terms_round_device(F, ts[:m], pt, n, te)
    assert g.shape == (D + 1, 4) and to_ints(g) == want, (n, "plain")
    assert all(np.array_equal(host(t), arrs[i]) for t, i in zip(ts, sel))   # a plain round only reads
    if host_form:
        hs = [arrs[i].copy() for i in sel]
        assert to_ints(multilinear.sumcheck_terms_round(F, hs[:m], pt, hs[m] if has_eq else None)) == want, (n, "host")
        assert all(np.array_equal(a, arrs[i]) for a, i in zip(hs, sel))
    if n < 2:
        return
    r_arr, bound = bound_case(name, n)
    want_f = T.round_poly(R, [bound[i] for i in range(m)], terms, bound[4] if has_eq else None)
    h = 1 << (n - 1)
    g = multilinear.sumcheck_terms_round_device(F, ts[:m], pt, n, te, r_arr)
    assert to_ints(g) == want_f, (n, "fused")
    for t, i in zip(ts, sel):
        assert to_ints(host(t)[:h]) == bound[i], (n, i)
    if host_form:   # the bound tables are written back to the first halves
        assert to_ints(multilinear.sumcheck_terms_round(F, hs[:m], pt, hs[m] if has_eq else None, r_arr)) == want_f, (n, "host fused")
        for a, i in zip(hs, sel):
            assert to_ints(a[:h]) == bound[i], (n, i)


@pytest.mark.parametrize("name", FIELDS)
@pytest.mark.parametrize("m,has_eq,tag", SHAPES)
def test_terms_round_matches_reference(name, m, has_eq, tag):
    terms = T.term_lists(F_REF[name], m, coeffs(name))[tag]
    for n in range(1, 15):
        _check_round(name, n, m, has_eq, terms, host_form=n <= 12)


@pytest.mark.parametrize("name", FIELDS)
@pytest.mark.parametrize("has_eq", [False, True])
@pytest.mark.parametrize("m", [1, 2, 3, 4])
def test_terms_round_2_18(name, m, has_eq):
    terms = T.term_lists(F_REF[name], m, coeffs(name))["A B - C" if m >= 3 else "all"]
    _check_round(name, 18, m, has_eq, terms, host_form=False)


@pytest.mark.parametrize("name", FIELDS)
@pytest.mark.parametrize("K", [1, 2, 3])
def test_one_term_equals_the_product_round_2_18(name, K):
    import torch
    from lambda_elliptic_curves_amd import multilinear
    F, n = fld(name), 18
    arrs, _ = case(name, n)
    r_arr, _ = bound_case(name, n)
    terms = [(None, tuple(range(K)))]
    t_prod, t_terms = [dev(a) for a in arrs[:K]], [dev(a) for a in arrs[:K]]
    for r in (None, r_arr):   # a plain round, then a fused one on the same tables
        g_prod = multilinear.sumcheck_round_device(F, t_prod, n, r)
        g_terms = multilinear.sumcheck_terms_round_device(F, t_terms, terms, n, None, r)
        assert np.array_equal(g_prod, g_terms)
        for a, b in zip(t_prod, t_terms):
            assert torch.equal(a[:1 << (n - 1)], b[:1 << (n - 1)])


@pytest.mark.parametrize("name", FIELDS)
def test_second_pair_per_thread_plain_2_20(name):
    from lambda_elliptic_curves_amd import multilinear
    R, n = F_REF[name], 20
    N, h = 1 << n, 1 << (n - 1)
    A = rand_elems(name, N, 3)
    ones = np.tile(to_arr([R.one]), (N, 1))
    s_lo, s_hi = limb_sum(A[:h]) % R.p, limb_sum(A[h:]) % R.p
    want = [((1 - u) * s_lo + u * s_hi) % R.p for u in range(3)]   # B = 1: g(u) = (1 - u) S_lo + u S_hi
    assert to_ints(multilinear.sumcheck_terms_round_device(fld(name), [dev(A), dev(ones)], [(None, (0, 1))], n)) == want


@pytest.mark.parametrize("name", FIELDS)
def test_second_pair_per_thread_fused_2_21(name):
    import torch
    from lambda_elliptic_curves_amd import multilinear
    R, n = F_REF[name], 21
    N, h, q = 1 << n, 1 << (n - 1), 1 << (n - 2)
    A = rand_elems(name, N, 4)
    one = to_arr([R.one])
    t_a, t_b, t_keep = dev(A), dev(np.tile(one, (N, 1))), dev(A)
    # r_prev = 1 binds every table to its upper half
    s_lo, s_hi = limb_sum(A[h:h + q]) % R.p, limb_sum(A[h + q:]) % R.p
    want = [((1 - u) * s_lo + u * s_hi) % R.p for u in range(3)]
    assert to_ints(multilinear.sumcheck_terms_round_device(fld(name), [t_a, t_b], [(None, (0, 1))], n, None, one[0])) == want
    assert torch.equal(t_a[:h], t_keep[h:])
    assert bool((t_b[:h] == dev(one)).all())


@pytest.mark.parametrize("name", FIELDS)
def test_operand_edges(name):
    from lambda_elliptic_curves_amd import multilinear
    F, R = fld(name), F_REF[name]
    p = R.p
    ones = ((1 << 256) - 1) % p   # limbs of all ones, reduced
    c_rnd = coeffs(name)[0]
    coeff_sets = {"0, 1": (0, R.one), "p - 1, -1": (p - 1, p - R.one), "random, all ones": (c_rnd, ones), "none": (None, None)}
    for n in (3, 10):
        N, h = 1 << n, 1 << (n - 1)
        rnd = case(name, n)[1][0]
        for tn, X in {"p - 1": [p - 1] * N, "all ones": [ones] * N, "zeros": [0] * N, "one": [R.one] * N}.items():
            for cn, (c0, c1) in coeff_sets.items():
                tag = (n, tn, cn)
                tabs, E = [X, list(X), rnd, list(X)], list(X)
                terms = [(c0, (0, 1, 2)), (c1, (3,)), (c1, (0, 3))]
                ts, te = [dev(to_arr(x)) for x in tabs], dev(to_arr(E))
                pt = py_terms(terms)
                assert to_ints(multilinear.sumcheck_terms_round_device(F, ts, pt, n, te)) == T.round_poly(R, tabs, terms, E), tag
                r = [p - 1, ones, R.one, c_rnd][(n + len(tn) + len(cn)) % 4]
                bound = [M.fix_variables(R, x, [r]) for x in tabs + [E]]
                g = multilinear.sumcheck_terms_round_device(F, ts, pt, n, te, to_arr([r])[0])
                assert to_ints(g) == T.round_poly(R, bound[:4], terms, bound[4]), tag
                assert [to_ints(host(x)[:h]) for x in ts + [te]] == bound, tag


# ---- proof ----
def _sha3_challenge(p):
    def ch(g):
        g = np.ascontiguousarray(g, dtype=np.uint64)
        return to_arr([int.from_bytes(hashlib.sha3_256(g.astype(">u8").tobytes()).digest(), "big") % p])[0]
    return ch


@pytest.mark.parametrize("name", FIELDS)
@pytest.mark.parametrize("n", [1, 2, 11])
def test_sumcheck_terms_prove_device(name, n):
    from lambda_elliptic_curves_amd import multilinear
    F, R = fld(name), F_REF[name]
    A, B = case(name, n)[1][:2]
    Cc = [R.mul(a, b) for a, b in zip(A, B)]
    tau = rand_elems(name, n, 600 + n)
    E = M.chis(R, to_ints(tau))
    terms = [(None, (0, 1)), (R.elem(R.p - 1), (2,))]   # eq (A B - C), C = A o B: the sum is zero
    ch = _sha3_challenge(R.p)
    t_eq = multilinear.eq_table_device(F, tau)
    got = multilinear.sumcheck_terms_prove_device(F, [dev(to_arr(x)) for x in (A, B, Cc)], py_terms(terms), n, ch, t_eq=t_eq)
    claimed, rounds, point, final = to_ints(got[0])[0], [to_ints(g) for g in got[1]], to_ints(got[2]), to_ints(got[3])
    assert claimed == 0
    assert len(rounds) == n and len(point) == n and len(final) == 4 and all(len(g) == 4 for g in rounds)
    # the same transcript as the honest Python prover, value for value
    assert (claimed, rounds, point, final) == T.prove(R, [A, B, Cc], terms, lambda g: to_ints(ch(to_arr(g)))[0], E)
    assert T.verify(R, terms, True, claimed, rounds, point, final)
    assert final == [M.evaluate(R, X, point) for X in (A, B, Cc, E)]
    assert final[3] == T.eq_closed_form(R, to_ints(tau), point)


@pytest.mark.parametrize("name", FIELDS)
def test_side_stream(name):
    import torch
    from lambda_elliptic_curves_amd import multilinear
    F, R, n = fld(name), F_REF[name], 13
    arrs, ints = case(name, n)
    r_arr, bound = bound_case(name, n)
    tau = rand_elems(name, n, 77)
    terms = T.term_lists(R, 3, coeffs(name))["A B - C"]
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        ts = [dev(a) for a in arrs[:3]] + [dev(arrs[4])]
        t_eq = torch.zeros((1 << n, 4), dtype=torch.int64, device="cuda")
        s.synchronize()
        multilinear.eq_table_device(F, tau, t_eq, stream=s.cuda_stream)
        g = multilinear.sumcheck_terms_round_device(F, ts[:3], py_terms(terms), n, ts[3], r_arr, stream=s.cuda_stream)   # synchronises: t_eq is complete too
    assert to_ints(host(t_eq)) == M.chis(R, to_ints(tau))
    assert to_ints(g) == T.round_poly(R, bound[:3], terms, bound[4])
