"""The Python restatement of PLONK rounds 1-3 (tests/plonk_rounds_ref.py) agrees with the rounds-1-3 flow that reaches the
reference's hard-coded commitments (tests/plonk_kat.py), on the CPU; blinding leaves the quotient unchanged; and the
lw_plonk_* entry points reject bad arguments before they touch a device."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from oracle import oracle as O
from tests import plonk_kat
from tests import plonk_kat_round45 as K45
from tests import plonk_rounds_ref as R
from tests import util

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_kats.json")


@pytest.fixture(scope="module")
def recorded():
    srs = util.plonk_test_srs(O.C_BLS12_381_G1, 7, 2)
    rec = K45.Recording(K45.OracleOps(srs))
    plonk_kat.rounds_1_to_3(rec, K45.omega())
    return srs, rec.polynomials()


@pytest.fixture(scope="module")
def restated():
    c = R.reference_test_circuit()
    f, n = c["field"], c["n"]
    p_abc = R.round_1(f, n, c["witness"])
    z, p_z = R.round_2(f, n, c["k1"], c["witness"], c["s_lagrange"], c["beta"], c["gamma"])
    t = R.round_3(f, n, c["k1"], c["q_coeffs"], c["s_coeffs"], p_abc, p_z, c["public_input"], c["beta"], c["gamma"], c["alpha"])
    return c, p_abc, z, p_z, t


def test_restatement_gives_the_polynomials_the_kat_flow_commits(recorded, restated):
    _, polys = recorded
    c, p_abc, _, p_z, t = restated
    f = c["field"]
    for name, got in zip(["p_a", "p_b", "p_c"], p_abc):
        assert R.strip(f, got) == polys[name], name
    assert R.strip(f, p_z) == polys["p_z"]
    for name, got in zip(["t_lo", "t_mid", "t_hi"], t):
        assert R.strip(f, got) == polys[name], name
    for name, got in zip(["ql", "qr", "qo", "qm", "qc"], c["q_coeffs"]):
        assert R.strip(f, got) == polys[name], name
    for name, got in zip(["s1", "s2", "s3"], c["s_coeffs"]):
        assert R.strip(f, got) == polys[name], name


def test_restatement_reaches_the_golden_round_2_and_3_commitments(recorded, restated):
    srs, _ = recorded
    c, _, _, p_z, t = restated
    with open(GOLDEN) as fh:
        want = json.load(fh)["plonk_round_2_3_commitments"]["expected"]
    commit = K45.OracleOps(srs).commit
    got = {"z_1": commit(R.strip(c["field"], p_z))}
    got.update({name: commit(R.strip(c["field"], blk)) for name, blk in zip(["t_lo_1", "t_mid_1", "t_hi_1"], t)})
    assert set(want) == set(got)
    for name, v in want.items():
        assert got[name] == (tuple(int(x, 16) for x in v) if v else None), name


@pytest.mark.parametrize("name", ["fr381", "stark252"])
def test_blinders_of_round_3_cancel_in_the_recombined_quotient(name):
    f = R.FIELDS[name]
    n = 8
    c = R.random_circuit(f, n, 5, n_pub=3)
    p_abc = R.round_1(f, n, c["witness"], blinders=[11, 12, 13, 14, 15, 16])
    _, p_z = R.round_2(f, n, c["k1"], c["witness"], c["s_lagrange"], c["beta"], c["gamma"], blinders=[21, 22, 23])
    args = (f, n, c["k1"], c["q_coeffs"], c["s_coeffs"], p_abc, p_z, c["public_input"], c["beta"], c["gamma"], c["alpha"])
    plain = R.round_3(*args)
    blind = R.round_3(*args, blinders=(f.p - 5, 77))
    assert blind != plain and blind[0][n + 2] == f.p - 5 and blind[1][n + 2] == 77

    def recombine(t):   # t_lo + X^(n+2) t_mid + X^(2n+4) t_hi
        out = [0] * (3 * n + 7)
        for k, blk in enumerate(t):
            for j, v in enumerate(blk):
                out[k * (n + 2) + j] = (out[k * (n + 2) + j] + v) % f.p
        return out
    assert recombine(blind) == recombine(plain)


def test_round_1_and_2_blinding_vanishes_on_the_domain():
    # p + (b0 + b1 X [+ b2 X^2]) (X^n - 1) takes the unblinded values on <w_n>, for n = 1 too
    f = R.FR381
    for n in (1, 2, 8):
        c = R.random_circuit(f, n, 9)
        w = R.omega(f, n)
        blinded = R.round_1(f, n, c["witness"], blinders=[3, 4, 5, 6, 7, 8])
        plain = R.round_1(f, n, c["witness"])
        for pb, pp, col in zip(blinded, plain, c["witness"]):
            assert len(pb) == n + 2 and pb != pp
            assert [K45.horner(pb, pow(w, i, f.p), f.p) for i in range(n)] == col
        z, p_z = R.round_2(f, n, c["k1"], c["witness"], c["s_lagrange"], c["beta"], c["gamma"], blinders=[1, 2, 3])
        assert len(p_z) == n + 3 and z[0] == 1
        assert [K45.horner(p_z, pow(w, i, f.p), f.p) for i in range(n)] == z


def test_plonk_entry_points_reject_bad_arguments_without_a_device():
    from lambda_elliptic_curves_amd import _lib as L
    lib = C.CDLL(L.LIB_PATH)   # a handle of its own: plain ctypes arguments, no argtypes
    buf = np.zeros(4096, np.uint8)
    P, N = C.c_void_p(buf.ctypes.data), C.c_void_p(None)
    i, sz = C.c_int, C.c_size_t
    S, FR, BB = i(0), i(1), i(2)
    h = C.c_void_p()
    H = C.byref(h)
    create = lib.lw_plonk_circuit_create
    cases = [
        ("create pow2", lambda: create(FR, sz(3), P, P, P, P, H), L.ERR_INPUT_NOT_POW2),
        ("create n 0", lambda: create(FR, sz(0), P, P, P, P, H), L.ERR_INPUT_NOT_POW2),
        ("create two-adicity", lambda: create(FR, sz(1 << 31), P, P, P, P, H), L.ERR_ROOT_OF_UNITY),   # 4n = 2^33 > 2^32
        ("create babybear", lambda: create(BB, sz(4), P, P, P, P, H), L.ERR_BAD_ARG),
        ("create field 7", lambda: create(i(7), sz(4), P, P, P, P, H), L.ERR_BAD_ARG),
        ("create null k1", lambda: create(S, sz(4), N, P, P, P, H), L.ERR_BAD_ARG),
        ("create null q", lambda: create(S, sz(4), P, N, P, P, H), L.ERR_BAD_ARG),
        ("create null s", lambda: create(S, sz(4), P, P, N, P, H), L.ERR_BAD_ARG),
        ("create null s_lagrange", lambda: create(S, sz(4), P, P, P, N, H), L.ERR_BAD_ARG),
        ("create null out", lambda: create(S, sz(4), P, P, P, P, N), L.ERR_BAD_ARG),
        # k1 = 0 (the buffer is all zeros): the coset offset has no inverse; decided on the host
        ("create k1 zero", lambda: create(FR, sz(4), P, P, P, P, H), L.ERR_INV_ZERO),
        ("round1 null circuit", lambda: lib.lw_plonk_round1(N, P, N, P), L.ERR_BAD_ARG),
        ("round1_device null circuit", lambda: lib.lw_plonk_round1_device(N, P, N, P, N), L.ERR_BAD_ARG),
        ("round2 null circuit", lambda: lib.lw_plonk_round2(N, P, P, P, N, N, P), L.ERR_BAD_ARG),
        ("round2_device null circuit", lambda: lib.lw_plonk_round2_device(N, P, P, P, N, N, P, N), L.ERR_BAD_ARG),
        ("round3 null circuit", lambda: lib.lw_plonk_round3(N, P, P, N, sz(0), P, P, P, N, P), L.ERR_BAD_ARG),
        ("round3_device null circuit", lambda: lib.lw_plonk_round3_device(N, P, P, N, sz(0), P, P, P, N, P, N), L.ERR_BAD_ARG),
    ]
    # k1 = 1 and k1 = w_4n: the vanishing polynomial has a root on the coset, also decided on the host
    for k1 in (1, R.omega(R.FR381, 16)):
        k = R.mont(R.FR381, [k1])
        cases.append((f"create k1^4n = 1 ({k1 == 1})", lambda k=k: create(FR, sz(4), C.c_void_p(k.ctypes.data), P, P, P, H), L.ERR_INV_ZERO))
    got = {name: call() for name, call, _ in cases}
    assert got == {name: code for name, _, code in cases}
    assert not h.value
    assert lib.lw_plonk_circuit_destroy(N) == 0
    # The checks that need a live handle (n_pub > n, a null or misaligned buffer with a good circuit) are in
    # tests/test_gpu_plonk.py: a handle holds device memory, so none can exist here.
