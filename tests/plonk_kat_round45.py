"""Restatement of the PLONK prover's rounds 4-5 for the reference test circuit (provers/plonk/src/prover.rs:537-626) in
Python big integers, on top of tests/plonk_kat.py's rounds 1-3.  A recording wrapper around the rounds-1-3 operations
captures the polynomials they interpolate and commit; round 4 evaluates them at zeta (Polynomial::evaluate), round 5
builds the seven polynomials of open_batch and the p_z opening at zeta * omega.  `Kzg` is the reference's
KateZaveruchaGoldberg::open / open_batch (crypto/src/commitments/kzg.rs:171-180, 206-226) over any commit function."""
import json
import os

import numpy as np

from oracle import oracle as O
from tests import plonk_kat

R = plonk_kat.R
N = plonk_kat.N
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "plonk_round_4_5.json")


def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def horner(coeffs, x, p=R):
    acc = 0
    for c in reversed(coeffs):
        acc = (acc * x + c) % p
    return acc


def ruffini(coeffs, x, p=R):
    """ruffini_division_inplace (math/src/polynomial/mod.rs:157-164): (quotient of n - 1 coefficients, popped remainder)"""
    c, q = 0, [0] * len(coeffs)
    for i in range(len(coeffs) - 1, -1, -1):
        q[i], c = c, (coeffs[i] + x * c) % p
    return q[:-1] if coeffs else [], c


def padd(*ps):
    out = [0] * max((len(p) for p in ps), default=0)
    for p in ps:
        for i, c in enumerate(p):
            out[i] = (out[i] + c) % R
    return out


def pscale(p, s):
    return [c * s % R for c in p]


def fold(polys, u):
    """open_batch's acc * upsilon + p over the reversed list: sum_k u^k p_k"""
    acc = []
    for p in reversed(polys):
        acc = padd(pscale(acc, u), p)
    return acc


class Kzg:
    def __init__(self, commit):
        self.commit = commit

    def open(self, x, y, p):
        q, _ = ruffini(padd(p, [(-y) % R]), x)
        return self.commit(q)

    def open_batch(self, x, ys, polys, u):
        acc_y = 0
        for y in reversed(ys):
            acc_y = (acc_y * u + y) % R
        return self.open(x, acc_y, fold(polys, u))


class Recording:
    """Wraps a rounds-1-3 ops object and keeps what rounds 4-5 read: the first eight interpolations are the circuit's
    selector and permutation polynomials (ql, qr, qo, qm, qc, s1, s2, s3), the commits are a, b, c, z, t_lo, t_mid, t_hi."""

    def __init__(self, ops):
        self.ops, self.interps, self.commits = ops, [], []

    def interp(self, evals):
        r = self.ops.interp(evals)
        self.interps.append(list(r))
        return r

    def eval_offset(self, coeffs, domain_size, offset):
        return self.ops.eval_offset(coeffs, domain_size, offset)

    def interp_offset(self, evals, offset):
        return self.ops.interp_offset(evals, offset)

    def commit(self, coeffs):
        self.commits.append(list(coeffs))
        return self.ops.commit(coeffs)

    def polynomials(self):
        names = ["ql", "qr", "qo", "qm", "qc", "s1", "s2", "s3"]
        out = {n: plonk_kat.strip(p) for n, p in zip(names, self.interps[:8])}
        out.update(zip(["p_a", "p_b", "p_c", "p_z", "t_lo", "t_mid", "t_hi"], self.commits[:7]))
        return out


class OracleOps:
    """tests/plonk_kat.py operations on the CPU oracle (canonical integers in and out)"""

    def __init__(self, srs):
        self.fr, self.oid, self.srs = O.F_FR381, O.C_BLS12_381_G1, srs

    def _m(self, v):
        return O.elems_to_mont(self.fr, v) if len(v) else np.zeros((0, 4), np.uint64)

    def interp(self, evals):
        return O.elems_from_mont(self.fr, O.interpolate_fft(self.fr, self._m(evals)))

    def eval_offset(self, coeffs, domain_size, offset):
        return O.elems_from_mont(self.fr, O.evaluate_fft(self.fr, self._m(coeffs), 1, domain_size, self._m([offset])[0]))

    def interp_offset(self, evals, offset):
        return O.elems_from_mont(self.fr, O.interpolate_fft(self.fr, self._m(evals), self._m([offset])[0]))

    def commit(self, coeffs):
        ks = O.ints_to_array(coeffs, 4) if coeffs else np.zeros((0, 4), np.uint64)
        return O.point_to_affine_ints(self.oid, O.msm(self.oid, ks, self.srs[:len(coeffs)]))


def omega():
    return O.elems_from_mont(O.F_FR381, [O.get_primitive_root_of_unity(O.F_FR381, 2)])[0]


def circuit_polynomials(srs):
    """rounds 1-3 on the oracle; -> {name: canonical coefficient list}"""
    rec = Recording(OracleOps(srs))
    plonk_kat.rounds_1_to_3(rec, omega())
    return rec.polynomials()


def round_4(polys, zeta, evaluate=None):
    """Round4Result (prover.rs:537-559): five polynomials at zeta, p_z at zeta * omega.  evaluate(coeffs_list, points)
    -> table [k][j]; default: Python Horner."""
    w = omega()
    evaluate = evaluate or (lambda ps, xs: [[horner(p, x) for x in xs] for p in ps])
    t = evaluate([polys["p_a"], polys["p_b"], polys["p_c"], polys["s1"], polys["s2"]], [zeta])
    zw = evaluate([polys["p_z"]], [zeta * w % R])
    return {"a_zeta": t[0][0], "b_zeta": t[1][0], "c_zeta": t[2][0], "s1_zeta": t[3][0], "s2_zeta": t[4][0],
            "z_zeta_omega": zw[0][0]}


def round_5_polynomials(polys, r4, zeta):
    """The seven polynomials round 5 opens at zeta (prover.rs:561-615)"""
    b, g, al, k1 = plonk_kat.BETA, plonk_kat.GAMMA, plonk_kat.ALPHA, plonk_kat.K1
    k2 = k1 * k1 % R
    a, bz, c = r4["a_zeta"], r4["b_zeta"], r4["c_zeta"]
    zeta_n = pow(zeta, N + 2, R)
    zeta_2n = pow(zeta, 2 * N + 4, R)
    l1 = (pow(zeta, N, R) - 1) * pow(zeta - 1, -1, R) * pow(N, -1, R) % R
    p_nc = padd(pscale(polys["qm"], a * bz % R), pscale(polys["ql"], a), pscale(polys["qr"], bz), pscale(polys["qo"], c), polys["qc"])
    r21 = pscale(polys["p_z"], (a + b * zeta + g) * (bz + b * k1 * zeta + g) * (c + b * k2 * zeta + g) % R)
    r22 = pscale(polys["s3"], (a + b * r4["s1_zeta"] + g) * (bz + b * r4["s2_zeta"] + g) * b * r4["z_zeta_omega"] % R)
    p_nc = padd(p_nc, pscale(padd(r22, pscale(r21, R - 1)), al))
    p_nc = padd(p_nc, pscale(polys["p_z"], l1 * al * al % R))
    partial_t = padd(polys["t_lo"], pscale(polys["t_mid"], zeta_n), pscale(polys["t_hi"], zeta_2n))
    return [partial_t, p_nc, polys["p_a"], polys["p_b"], polys["p_c"], polys["s1"], polys["s2"]]


def round_5(polys, r4, zeta, upsilon, kzg):
    """(w_zeta_1, w_zeta_omega_1) through kzg.open_batch / kzg.open"""
    ps = round_5_polynomials(polys, r4, zeta)
    ys = [horner(p, zeta) for p in ps]
    w1 = kzg.open_batch(zeta, ys, ps, upsilon)
    w2 = kzg.open(zeta * omega() % R, r4["z_zeta_omega"], polys["p_z"])
    return w1, w2
