"""A rank-one constraint system in plain Python integers: the restatement that the device code (lw_r1cs_*) is compared
with, from the definitions.  Elements are STORED values a R mod p over multilinear_ref.Fld(p, montgomery=True), so results
compare bit for bit.  A matrix is a CSR triple (row_ptr, col_idx, values) of Python lists; rows may be empty, columns
unsorted and repeated (they add up)."""
import json
import os

import numpy as np

from tests.multilinear_ref import MODULI, Fld  # noqa: F401
from tests.util import to_arr, to_ints  # noqa: F401

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def csr(n_rows, entries):
    """entries: (row, col, value) triples in any order -> (row_ptr, col_idx, values); a row keeps the order in which its
    entries were given"""
    rows = [[] for _ in range(n_rows)]
    for i, j, v in entries:
        rows[i].append((j, v))
    rp, ci, va = [0], [], []
    for r in rows:
        for j, v in r:
            ci.append(j)
            va.append(v)
        rp.append(len(ci))
    return rp, ci, va


def csr_arrays(mat):
    """a CSR triple of integers as the arrays R1cs() takes"""
    rp, ci, va = mat
    return np.array(rp, np.uint32), np.array(ci, np.uint32), to_arr(va)


def matvec(F, mat, z, n_out=None):
    """(M z)[i] = sum_k values[k] z[col_idx[k]] over row i; zeros up to n_out"""
    rp, ci, va = mat
    n_rows = len(rp) - 1
    out = [sum(F.mul(va[k], z[ci[k]]) for k in range(rp[i], rp[i + 1])) % F.p for i in range(n_rows)]
    return out + [0] * ((n_rows if n_out is None else n_out) - n_rows)


def bind_rows(F, mats, e, coeffs3, n_cols, n_out=None):
    """out[j] = sum_i e[i] (c_A A[i,j] + c_B B[i,j] + c_C C[i,j]); zeros up to n_out"""
    out = [0] * (n_cols if n_out is None else n_out)
    for (rp, ci, va), c in zip(mats, coeffs3):
        for i in range(len(rp) - 1):
            for k in range(rp[i], rp[i + 1]):
                out[ci[k]] = (out[ci[k]] + F.mul(e[i], F.mul(c, va[k]))) % F.p
    return out


def first_unsatisfied(F, mats, z):
    """the smallest i with (A z)_i (B z)_i != (C z)_i, or -1"""
    az, bz, cz = (matvec(F, m, z) for m in mats)
    for i, (a, b, c) in enumerate(zip(az, bz, cz)):
        if F.mul(a, b) != c:
            return i
    return -1


def dense(F, mat, n_cols):
    """the matrix as rows of stored values, repeated entries summed"""
    rp, ci, va = mat
    d = [[0] * n_cols for _ in range(len(rp) - 1)]
    for i in range(len(rp) - 1):
        for k in range(rp[i], rp[i + 1]):
            d[i][ci[k]] = (d[i][ci[k]] + va[k]) % F.p
    return d


# ---- the circom fixtures (tests/golden/circom_*.json: the data files of the reference's adapter tests)
def fixture(name):
    """-> (the r1cs dictionary, the witness as stored values) of 'vitalik' or 'poseidon', in circom's own column order"""
    F = Fld(MODULI["fr381"], True)
    r1 = json.load(open(os.path.join(GOLDEN, f"circom_{name}.r1cs.json")))
    w = json.load(open(os.path.join(GOLDEN, f"circom_{name}.witness.json")))
    return r1, [F.elem(int(v)) for v in w]


def circom_dense(F, r1):
    """The three dense matrices as the adapter's build_lro_from_circom_r1cs fills them (circom-adapter/src/lib.rs:33-63),
    before its input/output swap: l[var][constraint] = value, returned here as [constraint][var], stored values"""
    n_vars, n_gates = int(r1["nVars"]), int(r1["nConstraints"])
    lro = [[[0] * n_vars for _ in range(n_gates)] for _ in range(3)]
    for gate, constraint in enumerate(r1["constraints"]):
        for m in range(3):
            for var, dec in constraint[m].items():
                lro[m][gate][int(var)] = F.elem(int(dec))
    return lro


def circom_mats(F, r1):
    """CSR triples of integers straight from the dictionary"""
    mats = []
    for m in range(3):
        entries = [(gate, int(var), F.elem(int(dec))) for gate, con in enumerate(r1["constraints"]) for var, dec in con[m].items()]
        mats.append(csr(int(r1["nConstraints"]), entries))
    return mats
