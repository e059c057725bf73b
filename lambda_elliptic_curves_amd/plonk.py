"""PLONK prover rounds 1-3 on the device (provers/plonk/src/prover.rs:311-535, without the commitments) against a
device-resident circuit handle, the CommonPreprocessedInput of provers/plonk/src/setup.rs.  Elements are field elements
as stored (Montgomery form, (n, 4) uint64, MS limb first) over Stark252 or BLS12-381 Fr; challenges, k1, blinders and
the public input are host values in every form.  The device forms take and return torch tensors (int64, shape (len, 4)):
a round-1 / round-2 / round-3 block goes to msm.Srs.msm_fr_device for its commitment and to kzg.open_batch_device for
rounds 4-5 as it is."""
import ctypes as C

import numpy as np

from . import _lib as L
from .errors import check
from .poly import _elems, _one, _stream


def _opt(b, count):
    if b is None:
        return None, None
    a = _elems(b)
    if a.shape[0] != count:
        from .errors import LengthMismatch
        raise LengthMismatch(f"{a.shape[0]} blinders where {count} are taken")
    return a, a.ctypes.data_as(C.c_void_p)


def _vp(a):
    return a.ctypes.data_as(C.c_void_p)


class Circuit:
    """lw_plonk_circuit_*: built once per circuit from host arrays, like msm.Srs.  q_coeffs = (ql, qr, qo, qm, qc) and
    s_coeffs = (s1, s2, s3) in coefficient form (n each, zero padded), s_lagrange = the three permutation columns in
    evaluation form.  Holds 1376 n bytes on the device."""

    def __init__(self, field, n, k1, q_coeffs, s_coeffs, s_lagrange):
        self.field, self.n = field, int(n)
        self._h = C.c_void_p()
        q = np.concatenate([_elems(p) for p in q_coeffs]) if len(q_coeffs) else np.zeros((0, 4), np.uint64)
        s = np.concatenate([_elems(p) for p in s_coeffs]) if len(s_coeffs) else np.zeros((0, 4), np.uint64)
        sl = np.concatenate([_elems(p) for p in s_lagrange]) if len(s_lagrange) else np.zeros((0, 4), np.uint64)
        if q.shape[0] != 5 * self.n or s.shape[0] != 3 * self.n or sl.shape[0] != 3 * self.n:
            from .errors import LengthMismatch
            raise LengthMismatch("q_coeffs, s_coeffs, s_lagrange must hold 5, 3 and 3 columns of n elements")
        k = _one(k1)
        check(L.lib().lw_plonk_circuit_create(field.field, self.n, _vp(k), _vp(q), _vp(s), _vp(sl), C.byref(self._h)))

    # ---- host arrays
    def round1(self, witness, blinders=None):
        """witness: a | b | c, (3n, 4) -> p_a | p_b | p_c as a (3, n + 2, 4) array; blinders: (6, 4) or None."""
        w = _elems(witness)
        _b, bp = _opt(blinders, 6)
        out = np.zeros((3, self.n + 2, 4), np.uint64)
        self._rows(w, 3 * self.n)
        check(L.lib().lw_plonk_round1(self._h, _vp(w), bp, _vp(out)))
        return out

    def round2(self, witness, beta, gamma, blinders=None):
        """-> (z values (n, 4), p_z (n + 3, 4)); blinders: (3, 4) or None."""
        w = _elems(witness)
        self._rows(w, 3 * self.n)
        _b, bp = _opt(blinders, 3)
        be, ga = _one(beta), _one(gamma)
        z = np.zeros((self.n, 4), np.uint64)
        pz = np.zeros((self.n + 3, 4), np.uint64)
        check(L.lib().lw_plonk_round2(self._h, _vp(w), _vp(be), _vp(ga), bp, _vp(z), _vp(pz)))
        return z, pz

    def round3(self, p_abc, p_z, public_input, beta, gamma, alpha, blinders=None):
        """-> t_lo | t_mid | t_hi as a (3, n + 3, 4) array; blinders: (2, 4) = b_0, b_1 or None."""
        abc, pz = _elems(p_abc), _elems(p_z)
        self._rows(abc, 3 * (self.n + 2))
        self._rows(pz, self.n + 3)
        pi = _elems(public_input) if len(public_input) else np.zeros((0, 4), np.uint64)
        _b, bp = _opt(blinders, 2)
        be, ga, al = _one(beta), _one(gamma), _one(alpha)
        out = np.zeros((3, self.n + 3, 4), np.uint64)
        check(L.lib().lw_plonk_round3(self._h, _vp(abc), _vp(pz), _vp(pi) if pi.shape[0] else None, pi.shape[0], _vp(be), _vp(ga),
                                      _vp(al), bp, _vp(out)))
        return out

    # ---- torch tensors
    def round1_device(self, t_witness, blinders=None, stream=None):
        import torch
        _b, bp = _opt(blinders, 6)
        out = torch.empty((3, self.n + 2, 4), dtype=torch.int64, device=t_witness.device)
        self._rows(t_witness, 3 * self.n)
        check(L.lib().lw_plonk_round1_device(self._h, C.c_void_p(t_witness.data_ptr()), bp, C.c_void_p(out.data_ptr()), _stream(stream)))
        return out

    def round2_device(self, t_witness, beta, gamma, blinders=None, stream=None, z_values=False):
        """-> p_z (n + 3, 4), or (z values, p_z) with z_values=True.  Synchronises the stream once (the denominators'
        product is read back: a zero one raises errors.FieldError)."""
        import torch
        self._rows(t_witness, 3 * self.n)
        _b, bp = _opt(blinders, 3)
        be, ga = _one(beta), _one(gamma)
        pz = torch.empty((self.n + 3, 4), dtype=torch.int64, device=t_witness.device)
        z = torch.empty((self.n, 4), dtype=torch.int64, device=t_witness.device) if z_values else None
        check(L.lib().lw_plonk_round2_device(self._h, C.c_void_p(t_witness.data_ptr()), _vp(be), _vp(ga), bp,
                                             C.c_void_p(z.data_ptr()) if z_values else None, C.c_void_p(pz.data_ptr()), _stream(stream)))
        return (z, pz) if z_values else pz

    def round3_device(self, t_p_abc, t_p_z, public_input, beta, gamma, alpha, blinders=None, stream=None):
        import torch
        self._rows(t_p_abc, 3 * (self.n + 2))
        self._rows(t_p_z, self.n + 3)
        pi = _elems(public_input) if len(public_input) else np.zeros((0, 4), np.uint64)
        _b, bp = _opt(blinders, 2)
        be, ga, al = _one(beta), _one(gamma), _one(alpha)
        out = torch.empty((3, self.n + 3, 4), dtype=torch.int64, device=t_p_abc.device)
        check(L.lib().lw_plonk_round3_device(self._h, C.c_void_p(t_p_abc.data_ptr()), C.c_void_p(t_p_z.data_ptr()),
                                             _vp(pi) if pi.shape[0] else None, pi.shape[0], _vp(be), _vp(ga), _vp(al), bp,
                                             C.c_void_p(out.data_ptr()), _stream(stream)))
        return out

    @staticmethod
    def _rows(a, want):
        have = a.numel() // 4 if hasattr(a, "numel") else a.shape[0]
        if have != want:
            from .errors import LengthMismatch
            raise LengthMismatch(f"{have} elements where {want} are taken")

    def close(self):
        if self._h:
            L.lib().lw_plonk_circuit_destroy(self._h)
            self._h = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
