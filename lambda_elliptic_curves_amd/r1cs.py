"""A rank-one constraint system resident on the device (lw_r1cs_*): the three sparse matrices A, B, C over Stark252 or
BLS12-381 Fr, their products with a vector z (the tables of Spartan's first sumcheck, the evaluations Groth16 interpolates),
the row-bound combination M(r_x, .) of Spartan's second sumcheck, and the witness check.  Elements are field elements as
stored (Montgomery form, (n, 4) uint64, MS limb first); the device forms take and return torch tensors (int64, (len, 4))."""
import ctypes as C

import numpy as np

from . import _lib as L
from .errors import check
from ._lib import device_ptr, host_ptr, stream_ptr
from .multilinear import MODULI, _elems


def __getattr__(name):
    """SPLIT: entries of the longest list one work-item walks (longer lists are cut into pieces of SPLIT entries);
    TERMS: terms a Stark252 sum carries between two full reductions.  Both are read from the library."""
    if name == "SPLIT":
        return int(L.lib().lw_r1cs_split_length())
    if name == "TERMS":
        return int(L.lib().lw_r1cs_lazy_terms())
    raise AttributeError(name)


def _to_elems(field, ints):
    """integers -> stored elements v R mod p, (len, 4) uint64"""
    p = MODULI[field.field]
    out = np.zeros((len(ints), 4), np.uint64)
    for k, v in enumerate(ints):
        m = (int(v) % p) * (1 << 256) % p
        out[k] = [(m >> (64 * (3 - w))) & ((1 << 64) - 1) for w in range(4)]
    return out


def _csr(n_rows, mat):
    row_ptr, col_idx, values = mat
    rp = np.ascontiguousarray(row_ptr, dtype=np.uint32).reshape(-1)
    ci = np.ascontiguousarray(col_idx, dtype=np.uint32).reshape(-1)
    va = _elems(values) if np.size(values) else np.zeros((0, 4), np.uint64)
    if rp.shape[0] != n_rows + 1 or (rp.shape[0] and (ci.shape[0] != int(rp[-1]) or va.shape[0] != int(rp[-1]))):
        from .errors import LengthMismatch
        raise LengthMismatch(f"a CSR matrix of {n_rows} rows: row_ptr has {rp.shape[0]} entries, col_idx {ci.shape[0]}, values {va.shape[0]}")
    return rp, ci, va


def circom_csr(field, r1cs_dict):
    """circom's JSON form -> (n_rows, n_cols, [(row_ptr, col_idx, values)] * 3), host arrays only: what R1cs.from_circom
    hands to the constructor.  A row's entries keep the order of its map."""
    n_rows, n_cols = int(r1cs_dict["nConstraints"]), int(r1cs_dict["nVars"])
    mats = []
    for m in range(3):
        rp, ci, va = [0], [], []
        for row in r1cs_dict["constraints"]:
            for col, dec in row[m].items():
                ci.append(int(col))
                va.append(int(dec))
            rp.append(len(ci))
        mats.append((np.array(rp, np.uint32), np.array(ci, np.uint32), _to_elems(field, va)))
    return n_rows, n_cols, mats


class R1cs:
    """lw_r1cs_t: built once per circuit from three host CSR matrices (row_ptr, col_idx, values), like plonk.Circuit.
    Rows may be empty, columns unsorted, (row, column) pairs repeated (they add up)."""

    def __init__(self, field, n_rows, n_cols, matrices):
        self.field, self.n_rows, self.n_cols = field, int(n_rows), int(n_cols)
        self._h = C.c_void_p()
        if len(matrices) != 3:
            from .errors import LengthMismatch
            raise LengthMismatch("an R1CS has three matrices: A, B, C")
        keep = [_csr(self.n_rows, m) for m in matrices]
        arr = lambda k: (C.c_void_p * 3)(*[(m[k].ctypes.data if m[k].size else None) for m in keep])
        check(L.lib().lw_r1cs_create(field.field, self.n_rows, self.n_cols, arr(0), arr(1), arr(2), C.byref(self._h)))

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            try:
                L.lib().lw_r1cs_destroy(h)
            except Exception:
                pass

    @classmethod
    def from_dense(cls, field, a, b, c):
        """a, b, c: (n_rows, n_cols) tables of Python integers (residues); zeros are dropped."""
        n_rows, n_cols = len(a), len(a[0])
        mats = []
        for d in (a, b, c):
            rp, ci, va = [0], [], []
            for row in d:
                for j, v in enumerate(row):
                    if int(v) % MODULI[field.field]:
                        ci.append(j)
                        va.append(v)
                rp.append(len(ci))
            mats.append((rp, ci, _to_elems(field, va)))
        return cls(field, n_rows, n_cols, mats)

    @classmethod
    def from_circom(cls, r1cs_dict, field=None):
        """The JSON form circom writes (`snarkjs r1cs export json`): nVars, nConstraints and constraints as three
        {column: decimal} maps per row.  Circom's own column order is kept: the reference's adapter swaps inputs and
        outputs, which permutes z and the columns alike and changes no product.  BLS12-381 Fr unless a field is given."""
        if field is None:
            from .fft import FrField as field
        n_rows, n_cols, mats = circom_csr(field, r1cs_dict)
        return cls(field, n_rows, n_cols, mats)

    def _n_out(self, n_out, least):
        return least if n_out is None else int(n_out)

    def _vec(self, v, count, what):
        a = _elems(v)
        if a.shape[0] != count:
            from .errors import LengthMismatch
            raise LengthMismatch(f"{what} holds {a.shape[0]} elements, not {count}")
        return a

    # ---- host arrays
    def matvec(self, z, n_out=None, which=(True, True, True)):
        """-> [A z, B z, C z], each (n_out, 4) with zeros past n_rows (None where `which` is false); n_out >= n_rows."""
        zz = self._vec(z, self.n_cols, "z")
        n = self._n_out(n_out, self.n_rows)
        outs = [np.empty((max(n, 0), 4), np.uint64) if w else None for w in which]
        check(L.lib().lw_r1cs_matvec(self._h, host_ptr(zz), n, *[host_ptr(o) for o in outs]))
        return outs

    def bind_rows(self, e, coeffs3, n_out=None):
        """(n_out, 4): out[j] = sum_i e[i] (c_A A[i,j] + c_B B[i,j] + c_C C[i,j]), zeros past n_cols; n_out >= n_cols."""
        ee = self._vec(e, self.n_rows, "e")
        cc = self._vec(coeffs3, 3, "coeffs3")
        n = self._n_out(n_out, self.n_cols)
        out = np.empty((max(n, 0), 4), np.uint64)
        # an output of no element still has an address: n_out is what the library reports, not a null argument
        check(L.lib().lw_r1cs_bind_rows(self._h, host_ptr(ee), host_ptr(cc), n, C.c_void_p(out.ctypes.data)))
        return out

    def first_unsatisfied(self, z):
        """the smallest row i with (A z)_i (B z)_i != (C z)_i, or -1"""
        zz = self._vec(z, self.n_cols, "z")
        row = C.c_int64(0)
        check(L.lib().lw_r1cs_first_unsatisfied(self._h, host_ptr(zz), C.byref(row)))
        return int(row.value)

    # ---- device-resident tensors
    def matvec_device(self, t_z, n_out=None, t_out=(None, None, None), which=(True, True, True), stream=None):
        """matvec() of a device-resident z into t_out (tensors of n_out elements; allocated where None and asked for);
        nothing is waited for.  -> [t_az, t_bz, t_cz]"""
        import torch
        n = self._n_out(n_out, self.n_rows)
        outs = [(t if t is not None else torch.empty((n, 4), dtype=torch.int64, device=t_z.device)) if w else None
                for t, w in zip(t_out, which)]
        check(L.lib().lw_r1cs_matvec_device(self._h, device_ptr(t_z), n, *[device_ptr(o) if o is not None else None for o in outs],
                                            stream_ptr(stream)))
        return outs

    def bind_rows_device(self, t_e, coeffs3, n_out=None, t_out=None, stream=None):
        """bind_rows() of a device-resident e (the eq table of r_x) into t_out; nothing is waited for.  -> t_out"""
        import torch
        cc = self._vec(coeffs3, 3, "coeffs3")
        n = self._n_out(n_out, self.n_cols)
        if t_out is None:
            t_out = torch.empty((n, 4), dtype=torch.int64, device=t_e.device)
        check(L.lib().lw_r1cs_bind_rows_device(self._h, device_ptr(t_e), host_ptr(cc), n, device_ptr(t_out), stream_ptr(stream)))
        return t_out

    def first_unsatisfied_device(self, t_z, stream=None):
        row = C.c_int64(0)
        check(L.lib().lw_r1cs_first_unsatisfied_device(self._h, device_ptr(t_z), C.byref(row), stream_ptr(stream)))
        return int(row.value)
