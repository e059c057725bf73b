"""The group-law formulas of csrc/ec.cuh, one call per row through lw_hip_ec_pointwise_device, against plain Python
integers (tests/ec_formulas_ref.py) at operands the MSM never produces.

Every MSM, SRS and KZG test starts from on-curve points with pseudo-random coordinates and compares a normalised group
element: that pins the group law but not the arithmetic under it at large operands.  The complete formulas are
polynomials in the coordinates, so here every coordinate is chosen (p - 1 everywhere at once, limb-boundary values, the
operands that drive the unreduced sums of pt_add_mixed to their declared bounds) and the raw (X, Y, Z) are compared bit
for bit; every output coordinate must also be a canonical residue.

Reach of the targeted cases, sum of the products over p^2 at each product site of pt_add_mixed's device branch against
the KSUM fe_dot is told (profiles/ec_operand_bounds.txt; test_lazy_branch_at_its_declared_bounds asserts K - 0.05):
    BLS12-381 G1          mul_k<4> 4.0000 of 4   xo 2.9995 of 3   yo 4.9998 of 5   zo 6.9993 of 7
    BLS12-381 G1, b3 = 2  mul_k<4> 4.0000 of 4   xo 4.9999 of 5   yo 7.9975 of 8   zo 6.9998 of 7
    BN254 G1              mul_k<4> 4.0000 of 4   xo 2.9995 of 3   yo 3.9994 of 4   zo 4.9999 of 5
The best of the 4096 random tuples below stops 0.07 to 1.07 short of the dot products' bounds (zo: 5.93 of 7, 4.25 of 5).
"""
import functools
import itertools
import random

import numpy as np
import pytest

from oracle import oracle as O
from tests import ec_formulas_ref as E
from tests import util

pytestmark = pytest.mark.gpu
MODEL_IDS = [m.name for m in E.MODELS]
BY_NAME = {m.name: m for m in E.MODELS}
NCOORD = {E.OP_ADD: 6, E.OP_ADD_QUAD: 6, E.OP_ADD_MIXED: 5, E.OP_DBL: 3}


def lw_curve(m):
    from lambda_elliptic_curves_amd import msm
    return [msm.BLS12381Curve, msm.BN254Curve, msm.BN254TwistCurve, msm.BLS12381TwistCurve][m.curve]


def device_arrays(m, op, a, b, n, guard_rows=0):
    """the seam on packed arrays; guard_rows extra output rows are pre-filled and must come back untouched"""
    import torch
    from lambda_elliptic_curves_amd import msm
    cuda = lambda x: torch.from_numpy(np.ascontiguousarray(x).view(np.int64)).cuda()
    t_a, t_b = cuda(a), (cuda(b) if b is not None else None)
    out = torch.full((n + guard_rows, 3 * m.coord_words), 0x5a5a5a5a5a5a5a5a, dtype=torch.int64, device="cuda")
    msm.ec_pointwise_device(lw_curve(m), op, t_a, t_b, n, out, model=m.model)
    torch.cuda.synchronize()
    got = out.cpu().numpy().view(np.uint64)
    assert (got[n:] == np.uint64(0x5a5a5a5a5a5a5a5a)).all(), "rows past n were written"
    return got[:n]


def check_rows(m, op, a_rows, b_rows, want_rows):
    """device == reference, bit for bit, and every output coordinate below p"""
    got = device_arrays(m, op, E.pack_rows(m, a_rows), E.pack_rows(m, b_rows) if b_rows is not None else None, len(a_rows), guard_rows=1)
    flat = [v for r in E.unpack_rows(m, got) for c in r for v in (c if m.fp2 else (c,))]
    assert all(v < m.p for v in flat), "an output coordinate is not a canonical residue"
    want = E.pack_rows(m, want_rows)
    if not np.array_equal(got, want):
        i = int(np.nonzero((got != want).any(axis=1))[0][0])
        raise AssertionError(f"{m.name} op {op} row {i} of {len(a_rows)}: a = {a_rows[i]}, b = {b_rows[i] if b_rows else None}, "
                             f"got {E.unpack_rows(m, got[i:i + 1])[0]}, want {want_rows[i]}")


# ---------------------------------------------------------------- chosen coordinates
@functools.lru_cache(maxsize=None)
def edge_set(name):
    m = BY_NAME[name]
    return E.edge_values(m.p, m.words, 11)


def coord(m, c0, c1):
    return (c0, c1) if m.fp2 else c0


@functools.lru_cache(maxsize=None)
def tuples(name, kind, ncoord):
    """rows of ncoord stored coordinates"""
    m = BY_NAME[name]
    p, ed = m.p, edge_set(name)
    if kind == "exhaustive":      # every tuple over {0, 1, p - 1}; over Fp2 the same tuples with c1 = 0 and c1 = p - 1
        return [tuple(coord(m, v, c1) for v in t) for c1 in ((0, p - 1) if m.fp2 else (0,))
                for t in itertools.product((0, 1, p - 1), repeat=ncoord)]
    if kind == "all_equal":       # every coordinate (and component) the same member of E
        return [tuple(coord(m, e, e) for _ in range(ncoord)) for e in ed]
    rng = random.Random(1000 + ncoord)                            # 4096 tuples, each component from E or uniform, half and half
    draw = lambda: rng.choice(ed) if rng.random() < 0.5 else rng.randrange(p)
    return [tuple(coord(m, draw(), draw()) for _ in range(ncoord)) for _ in range(4096)]


@functools.lru_cache(maxsize=None)
def expected(name, op, kind):
    """the reference on tuples(name, kind, .), computed once; ADD_QUAD shares ADD's"""
    m = BY_NAME[name]
    rows = tuples(name, kind, NCOORD[op])
    return [E.stored_op(m, op, r[:3], r[3:] or None) for r in rows]


@pytest.mark.parametrize("kind", ["exhaustive", "all_equal", "random"])
@pytest.mark.parametrize("op", [E.OP_ADD, E.OP_ADD_MIXED, E.OP_DBL, E.OP_ADD_QUAD], ids=["add", "add_mixed", "dbl", "add_quad"])
@pytest.mark.parametrize("name", MODEL_IDS)
def test_formulas_bit_exact_at_chosen_coordinates(name, op, kind):
    m = BY_NAME[name]
    rows = tuples(name, kind, NCOORD[op])
    assert len(rows) == {"exhaustive": 3 ** NCOORD[op] * m.comps, "all_equal": len(edge_set(name)), "random": 4096}[kind]
    want = expected(name, E.OP_ADD if op == E.OP_ADD_QUAD else op, kind)
    check_rows(m, op, [r[:3] for r in rows], [r[3:] for r in rows] if op != E.OP_DBL else None, want)


@pytest.mark.parametrize("n", [1, 3, 16, 17, 4096 + 5])
@pytest.mark.parametrize("name", MODEL_IDS)
def test_quad_addition_gives_the_bytes_of_the_single_lane_addition(name, n):
    m = BY_NAME[name]
    rng = random.Random(n)
    ed = edge_set(name)
    draw = lambda: rng.choice(ed) if rng.random() < 0.5 else rng.randrange(m.p)
    rows = [tuple(coord(m, draw(), draw()) for _ in range(6)) for _ in range(n)]
    a, b = E.pack_rows(m, [r[:3] for r in rows]), E.pack_rows(m, [r[3:] for r in rows])
    single = device_arrays(m, E.OP_ADD, a, b, n, guard_rows=2)
    quad = device_arrays(m, E.OP_ADD_QUAD, a, b, n, guard_rows=2)      # n = 17: the last wave holds one quad
    assert np.array_equal(quad, single)
    k = min(n, 32)
    assert np.array_equal(single[:k], E.pack_rows(m, [E.stored_op(m, E.OP_ADD, r[:3], r[3:]) for r in rows[:k]]))


# ---------------------------------------------------------------- the unreduced sums of pt_add_mixed
@functools.lru_cache(maxsize=None)
def lazy_targets(name):
    return E.lazy_targets(BY_NAME[name])


@pytest.mark.parametrize("name", [m.name for m in E.MODELS if m.lazy])
def test_lazy_branch_at_its_declared_bounds(name):
    """Inputs that drive each of mul_k<4>, xo, yo and zo to the top of the range fe_dot was told (KSUM), and the corner
    t4 = 0 where fe_neg_raw_2p returns exactly 2p.  Coverage is asserted on the reference alone: every site has a case
    within 0.05 of its declared bound (reached: see the module docstring and profiles/ec_operand_bounds.txt), so a bound
    declared one unit too small, a dropped carry of add_nr or a wrong 2p - t4 changes the bytes compared below."""
    m = BY_NAME[name]
    tg = lazy_targets(name)
    rows = []
    for site in E.SITES:
        assert len(tg[site]) == E.N_KEEP
        top = max(E.lazy_shadow(m, *c)[0][site] for c in tg[site])
        print(f"{name} {site}: sum / p^2 = {float(top):.6f} of {E.LAZY_BOUNDS[name][site]}")
        assert top >= E.LAZY_BOUNDS[name][site] - 0.05, (name, site, float(top))
        assert top < E.LAZY_BOUNDS[name][site]
        rows += tg[site]
    for c in tg["corner"]:
        assert c[1] == 0 and (c[2] == 0 or c[4] == 0) and (c[3], c[4]) != (0, 0)      # t4 = 0 and q is not the identity row
    rows += tg["corner"]
    want = [E.stored_op(m, E.OP_ADD_MIXED, r[:3], r[3:]) for r in rows]
    assert all(E.lazy_shadow(m, *r)[1] == w for r, w in zip(rows, want))               # the shadow computes the same polynomial
    check_rows(m, E.OP_ADD_MIXED, [r[:3] for r in rows], [r[3:] for r in rows], want)


# ---------------------------------------------------------------- on-curve anchor: the Python formulas are the group law
def map_iso(m, row, u2, u3, back=False):
    """(X : Y : Z) -> (L^2 X : L^3 Y : Z) on stored coordinates (back: the inverse map)"""
    F = m.F
    if back:
        u2, u3 = F.inv(u2), F.inv(u3)
    x, y = (E.to_stored(m, F.mul(u, E.from_stored(m, c))) for u, c in ((u2, row[0]), (u3, row[1])))
    return (x, y) + tuple(row[2:])


@pytest.mark.parametrize("name", MODEL_IDS)
def test_on_curve_points_follow_the_oracle_group_law(name):
    """64 oracle points per curve through ADD, ADD_MIXED (q normalised by the oracle) and DBL, by affine equality with
    O.ec_add / O.ec_double, including P + P, P + (-P) and the identity on either side.  Model 1 gets its inputs through
    (x, y) -> (L^2 x, L^3 y) in Python, L^2 and L^3 derived from L^6, and its outputs through the inverse map."""
    m = BY_NAME[name]
    oid = m.curve
    _, pts = util.msm_case(oid, 64, 4242)
    idn = O.ec_neutral(oid)
    a = list(pts) + [pts[0], pts[1], idn, pts[2], idn]
    b = list(np.roll(pts, 1, axis=0)) + [pts[0], O.ec_neg(oid, pts[1]), pts[3], idn, idn]
    a_rows, b_rows = E.unpack_rows(m, np.stack(a)), E.unpack_rows(m, np.stack(b))
    b_aff = [r[:2] if r[2] != m.F.zero else (m.F.zero, m.F.zero) for r in E.unpack_rows(m, np.stack([O.ec_to_affine(oid, q) for q in b]))]
    if m.model:
        u2, u3 = E.iso_constants(m)
        a_rows, b_rows, b_aff = ([map_iso(m, r, u2, u3) for r in rows] for rows in (a_rows, b_rows, b_aff))   # (0, 0) stays (0, 0)
    sums = [O.point_to_affine_ints(oid, O.ec_add(oid, x, y)) for x, y in zip(a, b)]
    dbls = [O.point_to_affine_ints(oid, O.ec_double(oid, x)) for x in a]
    for op, second, want in ((E.OP_ADD, b_rows, sums), (E.OP_ADD_MIXED, b_aff, sums), (E.OP_DBL, None, dbls)):
        got = device_arrays(m, op, E.pack_rows(m, a_rows), E.pack_rows(m, second) if second else None, len(a_rows))
        ref = [E.stored_op(m, op, r, second[i] if second else None) for i, r in enumerate(a_rows)]
        assert np.array_equal(got, E.pack_rows(m, ref)), (name, op)
        rows = E.unpack_rows(m, got)
        if m.model:
            rows = [map_iso(m, r, u2, u3, back=True) for r in rows]
        back = E.pack_rows(m, rows)
        assert [O.point_to_affine_ints(oid, r) for r in back] == want, (name, op)


# ---------------------------------------------------------------- pt_to_affine: fe_inv_int_bingcd with a chosen Z
def norm_preimage(m, v):
    """(c0, c1), stored, whose stored norm fe_sqr(c0) + fe_sqr(c1) is v: the operand Fp2Ops::inv hands the binary GCD"""
    p = m.p
    for c1 in range(p):
        t = (v - c1 * c1 * m.Rinv) * m.R % p          # c0^2 / R = v - c1^2 / R
        c0 = pow(t, (p + 1) // 4, p)                  # p = 3 mod 4 for both base fields
        if c0 * c0 % p == t:
            return (c0, c1)


@pytest.mark.parametrize("name", MODEL_IDS)
def test_to_affine_inverts_a_chosen_z(name):
    """Z (for Fp2: its norm, the operand of the inversion, and Z = (z, 0), (0, z)) takes every non-zero member of E, 2^k,
    2^k +- 1 and p - 2^k for every bit k and 2000 values with p's top two limbs; X and Y are random.  Expected
    (X / Z, Y / Z, 1) with Python's pow(z, -1, p); Z = 0 gives (0 : 1 : 0)."""
    m = BY_NAME[name]
    p = m.p
    assert p % 4 == 3
    rng = random.Random(77)
    zs = E.inverse_operands(p, m.words, 5)
    assert len(zs) > 2000 + 3 * p.bit_length()
    if m.fp2:
        norms, zs = zs, [norm_preimage(m, v) for v in zs]
        assert all((c0 * c0 + c1 * c1) * m.Rinv % p == v for (c0, c1), v in zip(zs, norms))
        zs += [(z, 0) for z in edge_set(name) if z] + [(0, z) for z in edge_set(name) if z]
    zs = zs + [m.F.zero]
    r = lambda: coord(m, rng.randrange(p), rng.randrange(p))
    rows = [(r(), r(), z) for z in zs]
    want = [E.stored_op(m, E.OP_TO_AFFINE, row) for row in rows]
    assert want[-1] == (m.F.zero, E.stored_const(m, 1), m.F.zero)
    check_rows(m, E.OP_TO_AFFINE, rows, None, want)
