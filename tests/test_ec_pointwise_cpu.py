"""The group-law seam without a GPU: the argument checks of lw_hip_ec_pointwise_device, which all return before any
device work, and the reference of tests/test_gpu_ec_pointwise.py against the oracle's group law and against its own
coverage condition."""
import ctypes as C
import random

import numpy as np
import pytest

from oracle import oracle as O
from tests import ec_formulas_ref as E
from tests import util


@pytest.fixture(scope="module")
def lib():
    from lambda_elliptic_curves_amd import _lib
    return _lib, _lib.lib()


def test_pointwise_argument_checks(lib):
    L, dll = lib
    buf = np.zeros((4, 36), np.uint64)
    p = buf.ctypes.data_as(C.c_void_p)
    odd = C.c_void_p(buf.ctypes.data + 8)
    call = dll.lw_hip_ec_pointwise_device
    two = (L.EC_OP_ADD, L.EC_OP_ADD_MIXED, L.EC_OP_ADD_QUAD)
    for curve in (L.CURVE_BLS12_381_G1, L.CURVE_BN254_G1, L.CURVE_BN254_G2, L.CURVE_BLS12_381_G2):
        has_iso = curve in (L.CURVE_BLS12_381_G1, L.CURVE_BN254_G2)
        for op in range(5):
            b = p if op in two else None
            assert call(curve, 0, op, None, None, 0, None, None) == L.OK                     # n = 0: nothing touched, no device
            assert call(curve, 1, op, None, None, 0, None, None) == (L.OK if has_iso else L.ERR_BAD_ARG)
            assert call(curve, 0, op, None, b, 4, p, None) == L.ERR_BAD_ARG                  # null a
            assert call(curve, 0, op, p, b, 4, None, None) == L.ERR_BAD_ARG                  # null out
            assert call(curve, 0, op, p, None if op in two else p, 4, p, None) == L.ERR_BAD_ARG   # b missing / superfluous
            assert call(curve, 0, op, odd, b, 2, p, None) == L.ERR_BAD_ARG                   # misaligned
            assert call(curve, 2, op, p, b, 4, p, None) == L.ERR_BAD_ARG                     # no such model
            assert call(curve, -1, op, p, b, 4, p, None) == L.ERR_BAD_ARG
            if not has_iso:
                assert call(curve, 1, op, p, b, 4, p, None) == L.ERR_BAD_ARG
                assert b"model" in dll.lw_hip_last_error()
        assert call(curve, 0, 5, p, p, 4, p, None) == L.ERR_BAD_ARG                          # bad op
        assert call(curve, 0, -1, p, p, 4, p, None) == L.ERR_BAD_ARG
        assert call(curve, 0, 5, None, None, 0, None, None) == L.ERR_BAD_ARG                 # ... even with n = 0
    for curve in (4, -1):
        assert call(curve, 0, L.EC_OP_DBL, p, None, 4, p, None) == L.ERR_BAD_ARG             # bad curve
        assert call(curve, 0, L.EC_OP_DBL, None, None, 0, None, None) == L.ERR_BAD_ARG


@pytest.mark.parametrize("m", E.MODELS, ids=repr)
def test_reference_formulas_are_the_oracle_group_law(m):
    """Algorithms 7, 8 and 9 in Python against O.ec_add / O.ec_double on oracle points (P + P, P + (-P) and the identity
    included), model 1 through the isomorphism derived from L^6: the reference of the GPU test cannot be wrong in the
    same way as the kernel."""
    oid, F = m.curve, m.F
    _, pts = util.msm_case(oid, 16, 99)
    idn = O.ec_neutral(oid)
    a = list(pts) + [pts[0], pts[1], idn, pts[2], idn]
    b = list(np.roll(pts, 1, axis=0)) + [pts[0], O.ec_neg(oid, pts[1]), pts[3], idn, idn]
    a_rows, b_rows = E.unpack_rows(m, np.stack(a)), E.unpack_rows(m, np.stack(b))
    b_aff = [r[:2] if r[2] != F.zero else (F.zero, F.zero) for r in E.unpack_rows(m, np.stack([O.ec_to_affine(oid, q) for q in b]))]
    fwd = back = lambda r: r
    if m.model:
        u2, u3 = E.iso_constants(m)
        assert F.pow(u2, 3) == m.l6 and F.pow(u3, 2) == m.l6
        scale = lambda r, s2, s3: (E.to_stored(m, F.mul(s2, E.from_stored(m, r[0]))), E.to_stored(m, F.mul(s3, E.from_stored(m, r[1])))) + tuple(r[2:])
        fwd, back = (lambda r: scale(r, u2, u3)), (lambda r: scale(r, F.inv(u2), F.inv(u3)))
    aff = lambda rows: [O.point_to_affine_ints(oid, r) for r in E.pack_rows(m, [back(r) for r in rows])]
    sums = [O.point_to_affine_ints(oid, O.ec_add(oid, x, y)) for x, y in zip(a, b)]
    assert aff([E.stored_op(m, E.OP_ADD, fwd(x), fwd(y)) for x, y in zip(a_rows, b_rows)]) == sums
    assert aff([E.stored_op(m, E.OP_ADD_MIXED, fwd(x), fwd(y)) for x, y in zip(a_rows, b_aff)]) == sums
    assert aff([E.stored_op(m, E.OP_DBL, fwd(x)) for x in a_rows]) == [O.point_to_affine_ints(oid, O.ec_double(oid, x)) for x in a]
    assert aff([E.stored_op(m, E.OP_TO_AFFINE, fwd(x)) for x in a_rows]) == [O.point_to_affine_ints(oid, x) for x in a]


@pytest.mark.parametrize("m", [m for m in E.MODELS if m.lazy], ids=repr)
def test_targeted_cases_reach_the_declared_bounds_and_random_tuples_do_not(m):
    """The coverage condition of the GPU test on the reference alone, and why it takes targeted inputs: the best of 4096
    tuples drawn half from the edge set and half uniformly stays whole units below every bound the targeted cases touch."""
    tg = E.lazy_targets(m)
    ed = E.edge_values(m.p, m.words, 11)
    rng = random.Random(1005)
    draw = lambda: rng.choice(ed) if rng.random() < 0.5 else rng.randrange(m.p)
    rand = [E.lazy_shadow(m, *(draw() for _ in range(5)))[0] for _ in range(4096)]
    for site in ("xo", "yo", "zo"):
        K = E.LAZY_BOUNDS[m.name][site]
        top = max(E.lazy_shadow(m, *c)[0][site] for c in tg[site])
        top_rand = max(r[site] for r in rand)
        print(f"{m.name} {site}: targeted {float(top):.5f}, best of 4096 random {float(top_rand):.5f}, declared {K}")
        assert K - 0.05 <= top < K
        assert top_rand < top
    assert max(E.lazy_shadow(m, *c)[0]["mul4"] for c in tg["mul4"]) >= 4 - 0.05
    for c in [c for s in E.SITES for c in tg[s]] + tg["corner"]:
        assert E.lazy_shadow(m, *c)[1] == E.stored_op(m, E.OP_ADD_MIXED, c[:3], c[3:])
    for c in tg["corner"]:
        assert c[1] == 0 and (c[2] == 0 or c[4] == 0) and (c[3], c[4]) != (0, 0)          # t4 = 0: 2p - t4 is exactly 2p
