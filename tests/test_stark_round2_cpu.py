"""Round 2 without a GPU: the Python restatement (tests/stark_round2_ref.py) against the values the reference's
Stone-compatibility tests assert, break_in_parts' identity, and the argument checks of the new entry points, which all
return before any device work."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from oracle import bigint_def as D
from tests import stark_round2_ref as R2

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = D.P_STARK252


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(ROOT, "tests", "golden", "stark_round2.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def case1(golden):
    dom, lde, boundary, transitions, tevals = R2.fibonacci_2_cols_shifted_case(golden)
    evals = R2.evaluate(dom, lde, boundary, transitions, tevals)
    H = D.interpolate_fft_def(evals, P, dom.h)
    return dom, evals, H


def test_restatement_reproduces_the_stone_compat_composition_root(golden, case1):
    dom, _evals, H = case1
    blocks, lens = R2.break_in_parts(H, golden["n_parts"])
    assert sum(1 for c in H if c) == 3 and lens == [len(H) - next(i for i, c in enumerate(reversed(H)) if c)]
    lde = np.stack([R2.to_stored(P, R2.evaluate_on_coset(dom, b)) for b in blocks])
    nodes = R2.composition_nodes(lde)
    assert bytes(nodes[0]).hex() == golden["composition_root"]
    assert np.array_equal(nodes, R2.composition_nodes_by_rows(lde))


def test_restatement_reproduces_the_stone_compat_ood_evaluation(golden, case1):
    _dom, _evals, H = case1
    z, acc = int(golden["z"], 16), 0
    for c in reversed(H):
        acc = (acc * z + c) % P
    assert acc == int(golden["h0_at_z"], 16)


@pytest.mark.parametrize("n_parts", [2, 3, 4])
def test_break_in_parts_recomposes_on_the_lde_coset(n_parts):
    """sum_j x^j H_j(x^P) = H(x) at every LDE point, for an H with coefficients past P n (the thinning case)"""
    rng = np.random.default_rng(11 + n_parts)
    dom = R2.Domain(P, 2, 2, 3)
    H = [int.from_bytes(rng.bytes(31), "big") % P for _ in range(dom.N)]
    blocks, lens = R2.break_in_parts(H, n_parts)
    assert all(len(b) == len(blocks[0]) and len(b) & (len(b) - 1) == 0 for b in blocks) and lens == [len(H[j::n_parts]) for j in range(n_parts)]
    want = R2.evaluate_on_coset(dom, H)
    for i, x in enumerate(dom.coset):
        xp, got = pow(x, n_parts, P), 0
        for j, b in enumerate(blocks):
            acc = 0
            for c in reversed(b):
                acc = (acc * xp + c) % P
            got = (got + pow(x, j, P) * acc) % P
        assert got == want[i]


def test_zerofier_restatement_vanishes_where_the_constraint_applies():
    """E_c / Zc is the vanishing polynomial of the rows r = offset mod period, and E_c that of the exempted last rows:
    period 4, offset 1, two end exemptions at n = 16 (rows 8 and 12 by the reference's g^(n - k period))"""
    dom = R2.Domain(P, 4, 1, 3)
    t = dict(period=4, offset=1, end_exemptions=2, coeff=1)
    z = R2.zerofier_evaluations_on_extended_domain(dom, t)
    ee = R2.end_exemptions_evaluations(dom, t)
    den = D.interpolate_fft_def([e * pow(v, -1, P) % P for e, v in zip(ee, z)], P, dom.h)
    exm = D.interpolate_fft_def(ee, P, dom.h)
    at = lambda poly, x: sum(c * pow(x, k, P) for k, c in enumerate(poly)) % P
    for r in range(dom.n):
        x = pow(dom.g, r, P)
        assert (at(den, x) == 0) == (r % 4 == 1), r
        assert (at(exm, x) == 0) == (r in (8, 12)), r


# ---- argument checks through plain ctypes: every one returns before a device is needed

@pytest.fixture(scope="module")
def lib():
    from lambda_elliptic_curves_amd import _lib
    return _lib, _lib.lib()


def test_new_entry_points_are_exported(lib):
    L, dll = lib
    for name in ("lw_field_batch_inverse", "lw_field_batch_inverse_device", "lw_field_batch_inverse_block",
                 "lw_stark_constraint_evaluations_device", "lw_stark_composition_parts_device",
                 "lw_stark_commit_composition_device", "lw_stark_round2"):
        assert name in L.EXPORTS
        getattr(dll, name)
    assert dll.lw_field_batch_inverse_block() >= 64


def test_batch_inverse_argument_checks(lib):
    L, dll = lib
    buf = np.zeros((4, 4), np.uint64)
    p = buf.ctypes.data_as(C.c_void_p)
    assert dll.lw_field_batch_inverse(L.FIELD_STARK252, None, 0, None) == L.OK          # n = 0: no device
    assert dll.lw_field_batch_inverse_device(L.FIELD_BLS12_381_FR, None, 0, None, None) == L.OK
    assert dll.lw_field_batch_inverse(L.FIELD_BABYBEAR, p, 4, p) == L.ERR_BAD_ARG
    assert dll.lw_field_batch_inverse_device(L.FIELD_BABYBEAR, p, 4, p, None) == L.ERR_BAD_ARG
    assert dll.lw_field_batch_inverse(L.FIELD_STARK252, None, 4, p) == L.ERR_BAD_ARG
    assert dll.lw_field_batch_inverse(L.FIELD_STARK252, p, 4, None) == L.ERR_BAD_ARG
    assert dll.lw_field_batch_inverse_device(L.FIELD_STARK252, p, 4, None, None) == L.ERR_BAD_ARG


def _tables(L, period=1, col=0):
    b = (L.StarkBoundary * 1)()
    b[0].col, b[0].step = col, 0
    t = (L.StarkTransition * 1)()
    t[0].period = period
    return b, t


def test_constraint_evaluation_argument_checks(lib):
    L, dll = lib
    buf = np.zeros((16, 4), np.uint64)
    p = buf.ctypes.data_as(C.c_void_p)
    cols = (C.c_void_p * 1)(buf.ctypes.data)
    off = np.array([0, 0, 0, 3], np.uint64).ctypes.data_as(C.c_void_p)
    call = lambda field, cols, n_cols, lt, lb, off, b, nb, t, nt, tev, out: dll.lw_stark_constraint_evaluations_device(
        field, cols, n_cols, lt, lb, off, b, nb, t, nt, tev, 0, out, None)
    b, t = _tables(L)
    assert call(L.FIELD_BABYBEAR, cols, 1, 2, 2, off, b, 1, t, 1, p, p) == L.ERR_BAD_ARG
    assert call(L.FIELD_STARK252, cols, 1, 2, 2, None, b, 1, t, 1, p, p) == L.ERR_BAD_ARG        # null offset
    assert call(L.FIELD_STARK252, cols, 1, 2, 2, off, None, 1, t, 1, p, p) == L.ERR_BAD_ARG      # null boundary table
    assert call(L.FIELD_STARK252, cols, 1, 2, 2, off, b, 1, None, 1, p, p) == L.ERR_BAD_ARG      # null transition table
    assert call(L.FIELD_STARK252, cols, 1, 2, 2, off, b, 1, t, 1, None, p) == L.ERR_BAD_ARG      # null transition evaluations
    assert call(L.FIELD_STARK252, cols, 1, 2, 2, off, b, 1, t, 1, p, None) == L.ERR_BAD_ARG      # null output
    assert call(L.FIELD_STARK252, None, 1, 2, 2, off, b, 1, t, 1, p, p) == L.ERR_BAD_ARG         # null column table
    assert call(L.FIELD_STARK252, cols, 1, 30, 30, off, b, 1, t, 1, p, p) == L.ERR_BAD_ARG       # beyond the NTT
    assert call(L.FIELD_BLS12_381_FR, cols, 1, 20, 13, off, b, 1, t, 1, p, p) == L.ERR_BAD_ARG   # beyond the two-adicity
    b0, t0 = _tables(L, period=0)
    assert call(L.FIELD_STARK252, cols, 1, 2, 2, off, b0, 1, t0, 1, p, p) == L.ERR_BAD_ARG       # period = 0
    b1, t1 = _tables(L, col=1)
    assert call(L.FIELD_STARK252, cols, 1, 2, 2, off, b1, 1, t1, 1, p, p) == L.ERR_BAD_ARG       # col >= n_cols
    t1[0].end_exemptions = 5
    assert call(L.FIELD_STARK252, cols, 1, 2, 2, off, b, 1, t1, 1, p, p) == L.ERR_BAD_ARG        # more end exemptions than rows


def test_parts_and_commitment_argument_checks(lib):
    L, dll = lib
    buf = np.zeros((16, 4), np.uint64)
    p = buf.ctypes.data_as(C.c_void_p)
    off = np.array([0, 0, 0, 3], np.uint64).ctypes.data_as(C.c_void_p)
    parts = dll.lw_stark_composition_parts_device
    assert parts(L.FIELD_BABYBEAR, p, 4, off, 1, p, None, None, None) == L.ERR_BAD_ARG
    assert parts(L.FIELD_STARK252, p, 4, off, 0, p, None, None, None) == L.ERR_BAD_ARG       # P = 0
    assert parts(L.FIELD_STARK252, p, 4, off, 17, p, None, None, None) == L.ERR_BAD_ARG      # P > N
    assert parts(L.FIELD_STARK252, None, 4, off, 1, p, None, None, None) == L.ERR_BAD_ARG
    assert parts(L.FIELD_STARK252, p, 4, None, 1, p, None, None, None) == L.ERR_BAD_ARG
    assert parts(L.FIELD_STARK252, p, 4, off, 1, None, None, None, None) == L.ERR_BAD_ARG
    commit = dll.lw_stark_commit_composition_device
    assert commit(L.FIELD_BABYBEAR, p, 1, 0, 4, p, None, None) == L.ERR_BAD_ARG
    assert commit(L.FIELD_STARK252, None, 1, 0, 4, p, None, None) == L.ERR_BAD_ARG
    assert commit(L.FIELD_STARK252, p, 1, 0, 4, None, None, None) == L.ERR_BAD_ARG
    assert commit(L.FIELD_STARK252, p, 0, 0, 4, p, None, None) == L.ERR_BAD_ARG
    assert commit(L.FIELD_STARK252, p, 1, 0, 0, p, None, None) == L.ERR_BAD_ARG              # a single row has no pair
    b, t = _tables(L)
    lens = (C.c_size_t * 4)()
    root = np.zeros(32, np.uint8).ctypes.data_as(C.c_void_p)
    r2 = lambda field, n_parts, t, coeffs: dll.lw_stark_round2(field, p, 1, 1, 1, off, b, 1, t, 1, p, n_parts, coeffs, lens, root, None, None)
    assert r2(L.FIELD_BABYBEAR, 1, t, p) == L.ERR_BAD_ARG
    assert r2(L.FIELD_STARK252, 0, t, p) == L.ERR_BAD_ARG
    assert r2(L.FIELD_STARK252, 5, t, p) == L.ERR_BAD_ARG
    assert r2(L.FIELD_STARK252, 1, t, None) == L.ERR_BAD_ARG
    _b0, t0 = _tables(L, period=0)
    assert r2(L.FIELD_STARK252, 1, t0, p) == L.ERR_BAD_ARG
