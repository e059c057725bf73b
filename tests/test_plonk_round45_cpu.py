"""The Python restatement of PLONK rounds 4-5 (tests/plonk_kat_round45.py) reproduces the values the reference's
test_round_4 / test_round_5 hard-code, on the CPU; and the new evaluation / division / KZG entry points reject bad
arguments before they touch a device."""
import ctypes as C

import numpy as np
import pytest

from oracle import oracle as O
from tests import plonk_kat_round45 as K
from tests import util

H = lambda s: int(s, 16)


@pytest.fixture(scope="module")
def circuit():
    srs = util.plonk_test_srs(O.C_BLS12_381_G1, 7, 2)
    return srs, K.circuit_polynomials(srs)


def test_restatement_reproduces_round_4(circuit):
    _, polys = circuit
    g = K.golden()
    r4 = K.round_4(polys, H(g["challenges"]["zeta"]))
    for name, want in g["round_4"].items():
        if not name.startswith("_"):
            assert r4[name] == H(want), name


def test_restatement_reproduces_round_5(circuit):
    srs, polys = circuit
    g = K.golden()
    zeta, ups = H(g["challenges"]["zeta"]), H(g["challenges"]["upsilon"])
    r4 = K.round_4(polys, zeta)
    kzg = K.Kzg(K.OracleOps(srs).commit)
    w1, w2 = K.round_5(polys, r4, zeta, ups, kzg)
    assert w1 == tuple(H(v) for v in g["round_5"]["w_zeta_1"])
    assert w2 == tuple(H(v) for v in g["round_5"]["w_zeta_omega_1"])


def test_python_ruffini_matches_its_definition():
    rng = np.random.default_rng(3)
    p = K.R
    for n in (0, 1, 2, 5, 17):
        a = [int(v) for v in rng.integers(0, 1 << 62, n)]
        x = int(rng.integers(0, 1 << 62))
        q, rem = K.ruffini(a, x)
        assert len(q) == max(0, n - 1) and rem == K.horner(a, x)
        # a(X) = q(X) (X - x) + rem
        prod = [0] * max(n, 1)
        for i, c in enumerate(q):
            prod[i + 1] = (prod[i + 1] + c) % p
            prod[i] = (prod[i] - x * c) % p
        prod[0] = (prod[0] + rem) % p
        assert prod[:n] == [v % p for v in a] + [0] * (n - len(a))


def _lib():
    from lambda_elliptic_curves_amd import _lib
    return _lib


def test_poly_entry_points_reject_bad_arguments_without_a_device():
    L = _lib()
    lib = L.lib()
    a = np.ones((4, 4), np.uint64)
    x = np.ones(4, np.uint64)
    q = np.zeros((3, 4), np.uint64)
    vp = lambda arr: arr.ctypes.data_as(C.c_void_p)
    # BabyBear (or any non-4-limb field) is not taken
    assert lib.lw_poly_ruffini_division(L.FIELD_BABYBEAR, vp(a), 4, vp(x), vp(q), None) == L.ERR_BAD_ARG
    assert lib.lw_poly_ruffini_division(7, vp(a), 4, vp(x), vp(q), None) == L.ERR_BAD_ARG
    # null x, null coefficients, null quotient
    assert lib.lw_poly_ruffini_division(L.FIELD_STARK252, vp(a), 4, None, vp(q), None) == L.ERR_BAD_ARG
    assert lib.lw_poly_ruffini_division(L.FIELD_STARK252, None, 4, vp(x), vp(q), None) == L.ERR_BAD_ARG
    assert lib.lw_poly_ruffini_division(L.FIELD_STARK252, vp(a), 4, vp(x), None, None) == L.ERR_BAD_ARG
    # device form: the quotient overlaps the coefficients
    base = 1 << 20
    assert lib.lw_poly_ruffini_division_device(L.FIELD_STARK252, C.c_void_p(base), 4, vp(x), C.c_void_p(base + 32), None,
                                               None) == L.ERR_BAD_ARG
    assert lib.lw_poly_ruffini_division_device(L.FIELD_BLS12_381_FR, C.c_void_p(base), 4, vp(x), C.c_void_p(base + 8 + 4096),
                                               None, None) == L.ERR_BAD_ARG   # misaligned
    # n = 0 and n = 1 need no device: empty quotient, remainder 0 / a_0
    rem = np.full(4, 7, np.uint64)
    assert lib.lw_poly_ruffini_division(L.FIELD_STARK252, None, 0, vp(x), None, vp(rem)) == 0 and not rem.any()
    # evaluation: bad field, null points, null polynomial of non-zero length
    lens = (C.c_size_t * 1)(4)
    ptrs = (C.c_void_p * 1)(a.ctypes.data)
    out = np.zeros((1, 4), np.uint64)
    assert lib.lw_poly_evaluate(L.FIELD_BABYBEAR, ptrs, lens, 1, vp(x), 1, vp(out)) == L.ERR_BAD_ARG
    assert lib.lw_poly_evaluate(L.FIELD_STARK252, ptrs, lens, 1, None, 1, vp(out)) == L.ERR_BAD_ARG
    assert lib.lw_poly_evaluate(L.FIELD_STARK252, (C.c_void_p * 1)(None), lens, 1, vp(x), 1, vp(out)) == L.ERR_BAD_ARG
    # nothing to evaluate: no device either
    assert lib.lw_poly_evaluate(L.FIELD_STARK252, ptrs, lens, 1, vp(x), 0, None) == 0


def test_kzg_entry_points_reject_bad_arguments_without_a_device():
    L = _lib()
    lib = L.lib()
    from lambda_elliptic_curves_amd import errors, kzg
    a = np.ones((4, 4), np.uint64)
    x = np.ones(4, np.uint64)
    proof = np.zeros(18, np.uint64)
    vp = lambda arr: arr.ctypes.data_as(C.c_void_p)
    assert lib.lw_kzg_open(None, vp(a), 4, vp(x), vp(proof), None) == L.ERR_BAD_ARG      # no SRS
    # a batch of several polynomials needs upsilon; the checks run before the (null) SRS is dereferenced
    ptrs = (C.c_void_p * 2)(a.ctypes.data, a.ctypes.data)
    lens = (C.c_size_t * 2)(4, 4)
    assert lib.lw_kzg_open_batch(None, ptrs, lens, 2, vp(x), None, vp(proof), None) == L.ERR_BAD_ARG

    class _NoSrs:
        _h = C.c_void_p()
        curve = type("c", (), {"point_words": 18})()
    with pytest.raises(errors.HipError):
        kzg.open(_NoSrs(), a, x)
