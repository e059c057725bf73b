"""The resident R1CS without a GPU: every argument check lw_r1cs_create makes on the host, one bad argument at a time on
both fields; the checks of the compute calls that need no live handle; the circom parser against the dense matrices the
reference's adapter builds; the Python restatement (tests/r1cs_ref.py) on the fixtures' witnesses; no CPU fallback.

A handle holds device memory, so none can exist here: the checks that need a live one (n_out too small, overlapping
and misaligned buffers, with made-up addresses) are in tests/test_gpu_r1cs.py, as for lw_plonk_*."""
import ctypes as C

import numpy as np
import pytest

from tests import r1cs_ref as R

FIELDS = ["stark252", "fr381"]
FIELD_ID = {"stark252": 0, "fr381": 1}
SYMBOLS = ("lw_r1cs_create", "lw_r1cs_destroy", "lw_r1cs_split_length", "lw_r1cs_lazy_terms", "lw_r1cs_matvec", "lw_r1cs_matvec_device",
           "lw_r1cs_bind_rows", "lw_r1cs_bind_rows_device", "lw_r1cs_first_unsatisfied", "lw_r1cs_first_unsatisfied_device",
           "lw_groth16_h_from_witness", "lw_groth16_h_from_witness_device")


def fld(name):
    from lambda_elliptic_curves_amd import fft
    return {"stark252": fft.Stark252PrimeField, "fr381": fft.FrField}[name]


def test_symbols_are_exported_and_bound():
    from lambda_elliptic_curves_amd import _lib
    lib = _lib.lib()
    for s in SYMBOLS:
        assert s in _lib.EXPORTS and hasattr(lib, s)
        assert getattr(lib, s).argtypes is not None


def test_constants_are_those_of_the_accumulation_bound():
    from lambda_elliptic_curves_amd import r1cs
    p = R.MODULI["stark252"]
    # TERMS terms of less than 2p each fit eight limbs, one more need not
    assert 2 * r1cs.TERMS * p < 1 << 256 <= 2 * (r1cs.TERMS + 1) * p
    assert r1cs.SPLIT >= r1cs.TERMS
    with pytest.raises(AttributeError):
        r1cs.NO_SUCH_CONSTANT


@pytest.mark.parametrize("name", FIELDS)
def test_create_rejects_each_bad_argument(name):
    from lambda_elliptic_curves_amd import _lib as L
    lib = C.CDLL(L.LIB_PATH)   # a handle of its own: plain ctypes arguments, no argtypes
    F = R.Fld(R.MODULI[name], True)
    u32, N = C.c_uint32, C.c_void_p(None)
    fid = C.c_int(FIELD_ID[name])
    # a good 2 x 3 system: A = [[1, 0, 5], [0, 0, 0]], B = [[0, 1, 0], [1, 0, 0]], C empty
    rp = [np.array([0, 2, 2], np.uint32), np.array([0, 1, 2], np.uint32), np.array([0, 0, 0], np.uint32)]
    ci = [np.array([2, 0], np.uint32), np.array([1, 0], np.uint32), np.zeros(0, np.uint32)]
    va = [R.to_arr([F.elem(5), F.one]), R.to_arr([F.one, F.one]), np.zeros((0, 4), np.uint64)]

    def call(field=fid, n_rows=2, n_cols=3, rp=rp, ci=ci, va=va, null_arrays=(), out=True):
        ptr = lambda arrs, k: None if (k in null_arrays) else (C.c_void_p * 3)(*[(a.ctypes.data if a is not None and a.size else None) for a in arrs])
        h = C.c_void_p()
        rc = lib.lw_r1cs_create(field, u32(n_rows), u32(n_cols), ptr(rp, "rp"), ptr(ci, "ci"), ptr(va, "va"), C.byref(h) if out else N)
        assert not h.value or rc == 0
        if h.value:
            lib.lw_r1cs_destroy(h)
        return rc

    edit = lambda arrs, m, new: [new if k == m else a for k, a in enumerate(arrs)]
    p_arr, big = R.to_arr([F.p, F.one]), R.to_arr([(1 << 256) - 1, F.one])
    cases = {
        "field babybear": dict(field=C.c_int(2)),
        "field 7": dict(field=C.c_int(7)),
        "null row_ptr array": dict(null_arrays=("rp",)),
        "null col_idx array": dict(null_arrays=("ci",)),
        "null values array": dict(null_arrays=("va",)),
        "null out": dict(out=False),
        "null row_ptr[1]": dict(rp=edit(rp, 1, None)),
        "null col_idx[0] with entries": dict(ci=edit(ci, 0, None)),
        "null values[1] with entries": dict(va=edit(va, 1, None)),
        "no rows": dict(n_rows=0),
        "no columns": dict(n_cols=0),
        "rows above 2^30": dict(n_rows=(1 << 30) + 1),
        "columns above 2^30": dict(n_cols=(1 << 30) + 1),
        "row_ptr[0] != 0": dict(rp=edit(rp, 0, np.array([1, 2, 2], np.uint32))),
        "row_ptr decreases": dict(rp=edit(rp, 1, np.array([0, 2, 1], np.uint32))),
        "column == n_cols": dict(ci=edit(ci, 0, np.array([3, 0], np.uint32))),
        "column above": dict(ci=edit(ci, 1, np.array([1, 0xffffffff], np.uint32))),
        "value == p": dict(va=edit(va, 0, p_arr)),
        "value 2^256 - 1": dict(va=edit(va, 0, big)),
    }
    got = {k: call(**kw) for k, kw in cases.items()}
    assert got == {k: L.ERR_BAD_ARG for k in cases}
    # the good system passes every host check: what is left is the device
    import torch
    assert call() == (0 if torch.cuda.is_available() else L.ERR_NO_DEVICE)


def test_compute_calls_reject_null_arguments():
    from lambda_elliptic_curves_amd import _lib as L
    lib = C.CDLL(L.LIB_PATH)
    buf = np.zeros(4096, np.uint8)
    P, Q, N, sz = C.c_void_p(buf.ctypes.data), C.c_void_p(buf.ctypes.data + 2048), C.c_void_p(None), C.c_size_t
    row = C.c_int64(7)
    cases = [
        ("matvec", lambda: lib.lw_r1cs_matvec(N, P, sz(4), Q, N, N)),
        ("matvec_device", lambda: lib.lw_r1cs_matvec_device(N, P, sz(4), Q, N, N, N)),
        ("bind_rows", lambda: lib.lw_r1cs_bind_rows(N, P, P, sz(4), Q)),
        ("bind_rows_device", lambda: lib.lw_r1cs_bind_rows_device(N, P, P, sz(4), Q, N)),
        ("first_unsatisfied", lambda: lib.lw_r1cs_first_unsatisfied(N, P, C.byref(row))),
        ("first_unsatisfied_device", lambda: lib.lw_r1cs_first_unsatisfied_device(N, P, C.byref(row), N)),
        ("h_from_witness", lambda: lib.lw_groth16_h_from_witness(N, P, sz(4), Q, N)),
        ("h_from_witness_device", lambda: lib.lw_groth16_h_from_witness_device(N, P, sz(4), Q, N, N)),
    ]
    assert {k: f() for k, f in cases} == {k: L.ERR_BAD_ARG for k, _ in cases}
    assert row.value == 7
    assert lib.lw_r1cs_destroy(N) == 0


@pytest.mark.parametrize("fixture", ["vitalik", "poseidon"])
def test_circom_parser_matches_the_adapters_dense_matrices(fixture):
    from lambda_elliptic_curves_amd import r1cs
    F = R.Fld(R.MODULI["fr381"], True)
    r1, w = R.fixture(fixture)
    n_rows, n_cols, mats = r1cs.circom_csr(fld("fr381"), r1)
    assert (n_rows, n_cols) == (int(r1["nConstraints"]), int(r1["nVars"])) and len(w) == n_cols
    want = R.circom_dense(F, r1)
    for m, (rp, ci, va) in enumerate(mats):
        assert rp.dtype == np.uint32 and ci.dtype == np.uint32 and va.shape == (ci.shape[0], 4)
        assert R.dense(F, (rp.tolist(), ci.tolist(), R.to_ints(va)), n_cols) == want[m]
        assert [rp.tolist(), ci.tolist(), R.to_ints(va)] == list(R.circom_mats(F, r1)[m])


@pytest.mark.parametrize("fixture", ["vitalik", "poseidon"])
def test_reference_finds_the_fixture_witness_satisfied(fixture):
    F = R.Fld(R.MODULI["fr381"], True)
    r1, w = R.fixture(fixture)
    mats = R.circom_mats(F, r1)
    assert w[0] == F.one
    assert R.first_unsatisfied(F, mats, w) == -1
    bad = list(w)
    bad[len(bad) - 1] = (bad[-1] + 1) % F.p
    assert R.first_unsatisfied(F, mats, bad) >= 0


def test_reference_products_agree_with_each_other():
    """<e, cA Az + cB Bz + cC Cz> = <bind_rows(e), z> on a small system with empty rows, repeats and unsorted columns"""
    F = R.Fld(R.MODULI["stark252"], True)
    rng = np.random.default_rng(5)
    rnd = lambda: int.from_bytes(rng.bytes(40), "big") % F.p
    n_rows, n_cols = 7, 5
    mats = [R.csr(n_rows, [(int(rng.integers(1, n_rows - 1)), int(rng.integers(0, n_cols)), rnd()) for _ in range(12)]) for _ in range(3)]
    e, z, c3 = [rnd() for _ in range(n_rows)], [rnd() for _ in range(n_cols)], [rnd() for _ in range(3)]
    lhs = sum(F.mul(e[i], sum(F.mul(c, R.matvec(F, m, z)[i]) for c, m in zip(c3, mats)) % F.p) for i in range(n_rows)) % F.p
    rhs = sum(F.mul(b, zj) for b, zj in zip(R.bind_rows(F, mats, e, c3, n_cols), z)) % F.p
    assert lhs == rhs
    assert R.bind_rows(F, mats, e, c3, n_cols, 8)[n_cols:] == [0, 0, 0] and R.matvec(F, mats[0], z, 8)[n_rows:] == [0]


def test_no_cpu_fallback_without_device():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from lambda_elliptic_curves_amd import errors, r1cs
    F = R.Fld(R.MODULI["fr381"], True)
    r1, _ = R.fixture("vitalik")
    with pytest.raises(errors.HipError):
        r1cs.R1cs.from_circom(r1)
    with pytest.raises(errors.HipError):
        r1cs.R1cs.from_dense(fld("stark252"), [[1, 2]], [[0, 1]], [[3, 0]])
    with pytest.raises(errors.HipError):
        r1cs.R1cs(fld("fr381"), 1, 1, [R.csr_arrays(R.csr(1, [(0, 0, F.one)]))] * 3)
