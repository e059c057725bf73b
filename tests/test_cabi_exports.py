"""CPU-side checks of the drop-in boundary: the shared library loads and exports every symbol that
include/lw_hip.h declares; without a GPU every compute entry point fails loudly (no CPU fallback)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared_symbols():
    text = open(os.path.join(ROOT, "include", "lw_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(lw_[a-z0-9_]+)\s*\(", text)))


def test_library_exports_every_declared_symbol():
    from lambda_elliptic_curves_amd import _lib
    L = _lib.lib()
    declared = _declared_symbols()
    assert declared, "no declarations parsed"
    for sym in declared:
        assert hasattr(L, sym), f"{sym} declared in include/lw_hip.h but not exported"
    assert set(_lib.EXPORTS) == set(declared)


def test_no_cpu_fallback_without_device():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from lambda_elliptic_curves_amd import errors, fft, msm
    with pytest.raises(errors.HipError):
        fft.evaluate_fft(fft.Stark252PrimeField, np.ones((4, 4), np.uint64))
    with pytest.raises(errors.HipError):
        msm.msm(msm.BLS12381Curve, np.ones((1, 4), np.uint64), np.ones((1, 18), np.uint64))


def test_host_side_argument_checks_do_not_need_a_device():
    from lambda_elliptic_curves_amd import errors, fft, msm
    with pytest.raises(errors.InputError):
        fft.interpolate_fft(fft.Stark252PrimeField, np.ones((3, 4), np.uint64))
    with pytest.raises(errors.LengthMismatch):
        msm.msm(msm.BLS12381Curve, np.ones((2, 4), np.uint64), np.ones((1, 18), np.uint64))
    # zero polynomial: len zeros, no transform, no device needed (fft/polynomial.rs:33-35)
    z = fft.evaluate_fft(fft.Stark252PrimeField, np.zeros((3, 4), np.uint64), 2, 8)
    assert z.shape == (16, 4) and not z.any()
    # every C entry point, one bad argument at a time: the same code with or without a device
    from lambda_elliptic_curves_amd import _lib
    L = C.CDLL(_lib.LIB_PATH)   # a handle of its own: plain ctypes arguments, no argtypes
    buf = np.zeros(4096, np.uint8)
    P, Q, N = C.c_void_p(buf.ctypes.data), C.c_void_p(buf.ctypes.data + 2048), C.c_void_p(None)
    i, u32, sz = C.c_int, C.c_uint32, C.c_size_t
    S, FR, BB, U64, R32, EXT4, FWD = i(0), i(1), i(2), i(0), i(1), i(3), i(0)
    G1, BAD_CURVE = i(0), i(7)
    nttd = lambda f, l, lg, batch, stride, d_in: L.lw_hip_ntt_device(f, l, FWD, d_in, P, u32(lg), u32(batch), sz(stride), N, N)
    ntth = lambda f, l, lg, batch, stride, d_in: L.lw_hip_ntt(f, l, FWD, d_in, P, u32(lg), u32(batch), sz(stride), N)
    cross = lambda f, l, lg, d_in: L.lw_hip_ntt_cross_device(f, l, FWD, d_in, P, u32(lg), u32(1), sz(0), sz(8), sz(8), u32(1), sz(16), N)
    cases = []
    for name, ntt in (("ntt", ntth), ("ntt_device", nttd)):
        cases += [
            (name + " layout", lambda ntt=ntt: ntt(S, R32, 4, 1, 0, P), _lib.ERR_BAD_ARG),
            (name + " order 64", lambda ntt=ntt: ntt(S, U64, 64, 1, 0, P), _lib.ERR_ORDER_TOO_LARGE),
            (name + " root", lambda ntt=ntt: ntt(FR, U64, 33, 1, 0, P), _lib.ERR_ROOT_OF_UNITY),
            (name + " stride", lambda ntt=ntt: ntt(S, U64, 4, 2, 8, P), _lib.ERR_BAD_ARG),
            (name + " null", lambda ntt=ntt: ntt(S, U64, 4, 1, 0, N), _lib.ERR_BAD_ARG),
        ]
    cases += [
        ("ntt_lde_device layout", lambda: L.lw_hip_ntt_lde_device(S, EXT4, P, u32(2), P, u32(4), u32(1), N, N), _lib.ERR_BAD_ARG),
        ("ntt_lde_device order 64", lambda: L.lw_hip_ntt_lde_device(S, U64, P, u32(2), P, u32(64), u32(1), N, N), _lib.ERR_ORDER_TOO_LARGE),
        ("ntt_lde_device null", lambda: L.lw_hip_ntt_lde_device(S, U64, N, u32(2), P, u32(4), u32(1), N, N), _lib.ERR_BAD_ARG),
        ("ntt_cross_device layout", lambda: cross(S, R32, 4, P), _lib.ERR_BAD_ARG),
        ("ntt_cross_device order 64", lambda: cross(S, U64, 64, P), _lib.ERR_ORDER_TOO_LARGE),
        ("ntt_cross_device null", lambda: cross(S, U64, 4, N), _lib.ERR_BAD_ARG),
        ("bitrev pow2", lambda: L.lw_hip_bitrev_permutation(S, U64, P, P, sz(3)), _lib.ERR_INPUT_NOT_POW2),
        ("interpolate pow2", lambda: L.lw_polynomial_interpolate_fft(S, U64, P, sz(3), N, P, N), _lib.ERR_INPUT_NOT_POW2),
        ("fri_layer pow2", lambda: L.lw_stark_fri_layer(S, P, sz(4), P, P, sz(6), P, N, P, P, N), _lib.ERR_INPUT_NOT_POW2),
        ("fri_layer_device pow2", lambda: L.lw_stark_fri_layer_device(S, P, sz(4), P, P, sz(6), Q, N, P, N, N), _lib.ERR_INPUT_NOT_POW2),
        ("fri_layer field", lambda: L.lw_stark_fri_layer(BB, P, sz(4), P, P, sz(8), P, N, P, P, N), _lib.ERR_BAD_ARG),
        ("groth16_h pow2", lambda: L.lw_groth16_h_coefficients(P, P, P, sz(2), sz(3), P, N), _lib.ERR_INPUT_NOT_POW2),
        ("groth16_h_device pow2", lambda: L.lw_groth16_h_coefficients_device(P, P, P, sz(2), sz(3), P, N, N), _lib.ERR_INPUT_NOT_POW2),
        ("groth16_h null", lambda: L.lw_groth16_h_coefficients(N, P, P, sz(0), sz(4), P, N), _lib.ERR_BAD_ARG),
        ("msm_limbs 0", lambda: L.lw_hip_msm_limbs(G1, P, u32(0), sz(1), P, sz(1), P), _lib.ERR_BAD_ARG),
        ("msm_limbs 9", lambda: L.lw_hip_msm_limbs(G1, P, u32(9), sz(1), P, sz(1), P), _lib.ERR_BAD_ARG),
        ("msm_limbs_device 0", lambda: L.lw_hip_msm_limbs_device(G1, P, u32(0), P, sz(1), P, N), _lib.ERR_BAD_ARG),
        ("msm_limbs_device 9", lambda: L.lw_hip_msm_limbs_device(G1, P, u32(9), P, sz(1), P, N), _lib.ERR_BAD_ARG),
        ("msm curve", lambda: L.lw_hip_msm(BAD_CURVE, P, sz(1), P, sz(1), P), _lib.ERR_BAD_ARG),
        ("msm_device curve", lambda: L.lw_hip_msm_device(BAD_CURVE, P, P, sz(1), P, N), _lib.ERR_BAD_ARG),
        ("msm_fr_device curve", lambda: L.lw_hip_msm_fr_device(BAD_CURVE, P, P, sz(1), P, N), _lib.ERR_BAD_ARG),
        ("msm lengths", lambda: L.lw_hip_msm(G1, P, sz(2), P, sz(1), P), _lib.ERR_LENGTH_MISMATCH),
        ("msm null", lambda: L.lw_hip_msm(G1, N, sz(1), P, sz(1), P), _lib.ERR_BAD_ARG),
        ("srs_create curve", lambda: L.lw_hip_srs_create(BAD_CURVE, P, sz(1), P), _lib.ERR_BAD_ARG),
        ("srs_create_device curve", lambda: L.lw_hip_srs_create_device(BAD_CURVE, P, sz(1), N, P), _lib.ERR_BAD_ARG),
        ("ec_add_outer_device curve", lambda: L.lw_hip_ec_add_outer_device(BAD_CURVE, P, sz(1), P, sz(1), P, N), _lib.ERR_BAD_ARG),
        ("commit_columns field", lambda: L.lw_stark_commit_columns(BB, P, u32(1), u32(2), i(0), P, N), _lib.ERR_BAD_ARG),
        ("commit_columns leaves", lambda: L.lw_stark_commit_columns(S, P, u32(1), u32(32), i(0), P, N), _lib.ERR_ALLOC),
        ("commit_columns_device field", lambda: L.lw_stark_commit_columns_device(BB, P, u32(1), sz(0), u32(2), i(0), P, N, N), _lib.ERR_BAD_ARG),
        ("commit_columns_device row bytes", lambda: L.lw_stark_commit_columns_device(S, P, u32(1 << 26), sz(0), u32(0), i(0), P, N, N), _lib.ERR_BAD_ARG),
        ("commit_columns_layout_device ext4", lambda: L.lw_stark_commit_columns_layout_device(BB, EXT4, P, u32(1), sz(0), u32(2), i(0), P, N, N), _lib.ERR_BAD_ARG),
        ("commit_columns_layout_device null", lambda: L.lw_stark_commit_columns_layout_device(BB, R32, N, u32(1), sz(0), u32(2), i(0), P, N, N), _lib.ERR_BAD_ARG),
        ("commit_columns_device column stride", lambda: L.lw_stark_commit_columns_device(S, P, u32(2), sz(3), u32(2), i(0), Q, N, N), _lib.ERR_BAD_ARG),
        ("commit_columns_layout_device column stride", lambda: L.lw_stark_commit_columns_layout_device(BB, R32, P, u32(2), sz(3), u32(2), i(0), Q, N, N), _lib.ERR_BAD_ARG),
    ]
    got = {name: call() for name, call, _ in cases}
    assert got == {name: code for name, _, code in cases}


def test_commit_wrappers_pass_the_column_stride_on():
    """col_stride_elems of the two Keccak wrappers reaches the C entry: a stride below the column length comes back as that
    entry's refusal, which is made before any device work (the pointers are host memory and are never followed)."""
    from lambda_elliptic_curves_amd import errors, fft, merkle

    class Buffer:
        def __init__(self, nbytes):
            self.a = np.zeros(nbytes, np.uint8)

        def data_ptr(self):
            return self.a.ctypes.data

    cols, nodes = Buffer(2 * 4 * 32), Buffer(7 * 32)
    for call, fld in ((merkle.commit_columns_device, fft.Stark252PrimeField), (merkle.commit_columns_device, fft.FrField),
                      (merkle.commit_columns_layout_device, fft.Babybear31PrimeFieldU32), (merkle.commit_columns_layout_device, fft.Babybear31PrimeField)):
        with pytest.raises(errors.HipError, match="column stride 3 below the column length"):
            call(fld, cols, 2, 2, nodes, col_stride_elems=3, stream=0)
    assert not cols.a.any() and not nodes.a.any()


def test_product_never_touches_the_oracle():
    pkg = os.path.join(ROOT, "lambda_elliptic_curves_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".cuh", ".h", ".cpp")):
                text = open(os.path.join(dirpath, f), errors="replace").read()
                assert "oracle" not in text.lower().replace("no cpu fallback", ""), f"{f} mentions the oracle"


def test_tools_do_not_use_the_checker():
    # oracle/ is test infrastructure: only tests/, __graft_entry__.smoke() and bench.py's cpu_baseline legs may import it
    # (tests/util.py does, so the tools take their inputs from tools/inputs.py instead)
    for f in sorted(os.listdir(os.path.join(ROOT, "tools"))):
        if f.endswith(".py"):
            text = open(os.path.join(ROOT, "tools", f)).read()
            assert not re.search(r"^\s*(from|import)\s+(oracle|tests)\b", text, re.M), f"tools/{f} imports the checker"


def test_rust_shim_declares_every_symbol_and_status():
    # rust-shim/src/ffi.rs cannot be compiled here (no Rust toolchain); at least keep it in step with the header
    ffi = open(os.path.join(ROOT, "rust-shim", "src", "ffi.rs")).read()
    declared = set(_declared_symbols())
    assert set(re.findall(r"pub fn (lw_[a-z0-9_]+)\s*\(", ffi)) == declared
    header = open(os.path.join(ROOT, "include", "lw_hip.h")).read()
    for name, val in re.findall(r"\b(LW_(?:OK|ERR_[A-Z0-9_]+))\s*=\s*(-?\d+)", header):
        assert re.search(r"pub const %s: c_int = %s;" % (name, val), ffi), name
    for enum, variants in (("lw_field_t", 3), ("lw_layout_t", 4), ("lw_curve_t", 4)):
        body = re.search(r"typedef enum \{([^}]*)\} %s;" % enum, header, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        assert len(re.findall(r"=\s*\d+", body)) == variants
