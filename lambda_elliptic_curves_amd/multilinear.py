"""DenseMultilinearPolynomial::evaluate / fix_variables (math/src/polynomial/dense_multilinear_poly.rs) and the prover's
round of a sumcheck over a product of K tables, on the device, over Stark252 and BLS12-381 Fr.  A table is a (2^n, 4)
uint64 array in the reference's memory form (Montgomery, MS limb first); variable x_0 is the MOST significant bit of the
index.  Points and challenges are host values in every form.  The transcript stays with the caller."""
import ctypes as C

import numpy as np

from . import _lib as L
from .errors import check

MODULI = {
    L.FIELD_STARK252: 0x800000000000011000000000000000000000000000000000000000000000001,
    L.FIELD_BLS12_381_FR: 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001,
}


def _elems(a):
    return np.ascontiguousarray(a, dtype=np.uint64).reshape(-1, 4)


def _opt(r):
    """one optional host element -> (array kept alive, pointer or None)"""
    if r is None:
        return None, None
    a = np.ascontiguousarray(r, dtype=np.uint64).reshape(-1)[:4].copy()
    return a, L.host_ptr(a)


def _ptrs(addresses):
    """the pointer array of a call's tables (one slot even for none: the library reports the count itself)"""
    return (C.c_void_p * max(1, len(addresses)))(*addresses)


def _bound_in_place(r_prev, arrays):
    """a fused host round writes the bound tables into the caller's arrays, so they must be what the library is given"""
    ok = lambda u: isinstance(u, np.ndarray) and u.dtype == np.uint64 and u.flags.c_contiguous and u.flags.writeable
    if r_prev is not None and not all(ok(u) for u in arrays):
        from .errors import InputError
        raise InputError("a fused round binds in place: pass C-contiguous uint64 arrays")


def _n_vars(table):
    n = table.shape[0]
    if n == 0 or n & (n - 1):
        from .errors import InputError
        raise InputError(f"a multilinear table has 2^n elements, not {n}")
    return n.bit_length() - 1


def _point(point, n):
    p = _elems(point) if n else np.zeros((1, 4), np.uint64)
    if n and p.shape[0] != n:
        from .errors import LengthMismatch
        raise LengthMismatch(f"{p.shape[0]} coordinates for {n} variables")
    return p


def evaluate(field, tables, point):
    """(K, 4): tables[k] at `point` (n elements for tables of 2^n); every table has the same size."""
    ts = [_elems(t) for t in tables]
    n = _n_vars(ts[0]) if ts else 0
    p = _point(point, n)
    out = np.zeros((len(ts), 4), np.uint64)
    check(L.lib().lw_multilinear_evaluate(field.field, _ptrs([t.ctypes.data for t in ts]), len(ts), n, L.host_ptr(p), L.host_ptr(out)))
    return out


def evaluate_device(field, t_tables, n_vars, point, stream=None):
    """evaluate() on device-resident torch tensors of at least 2^n_vars elements each."""
    p = _point(point, n_vars)
    out = np.zeros((len(t_tables), 4), np.uint64)
    check(L.lib().lw_multilinear_evaluate_device(field.field, _ptrs([t.data_ptr() for t in t_tables]), len(t_tables), n_vars, L.host_ptr(p),
                                                 L.host_ptr(out), L.stream_ptr(stream)))
    return out


def fix_variables(field, table, r):
    """(2^(n - t), 4): the table with its first t = len(r) variables bound to r."""
    a = _elems(table)
    n = _n_vars(a)
    rr = _elems(r) if len(r) else np.zeros((0, 4), np.uint64)
    t = rr.shape[0]
    out = np.zeros((1 << max(0, n - t), 4), np.uint64)
    check(L.lib().lw_multilinear_fix_variables(field.field, L.host_ptr(a), n, L.host_ptr(rr), t, L.host_ptr(out)))
    return out


def fix_variables_device(field, t_table, n_vars, r, t_out, stream=None):
    """fix_variables() of a device-resident tensor into t_out (2^(n_vars - len(r)) elements, not overlapping t_table);
    nothing is waited for.  -> t_out"""
    rr = _elems(r) if len(r) else np.zeros((0, 4), np.uint64)
    check(L.lib().lw_multilinear_fix_variables_device(field.field, L.device_ptr(t_table), n_vars, L.host_ptr(rr), rr.shape[0],
                                                      L.device_ptr(t_out), L.stream_ptr(stream)))
    return t_out


def sumcheck_round(field, tables, r_prev=None):
    """(K + 1, 4): g(0) .. g(K) of the round over K = 1, 2 or 3 tables of 2^n elements.  With r_prev the tables (which
    must then be writable (2^n, 4) uint64 arrays) are first bound to it in place - their first halves hold the bound
    tables afterwards - and the round runs over the n - 1 remaining variables."""
    ts = [_elems(t) for t in tables]
    _bound_in_place(r_prev, tables)
    n = _n_vars(ts[0]) if ts else 0
    out = np.zeros((len(ts) + 1, 4), np.uint64)
    keep, rp = _opt(r_prev)
    check(L.lib().lw_sumcheck_round(field.field, _ptrs([t.ctypes.data for t in ts]), len(ts), n, rp, L.host_ptr(out)))
    return out


def sumcheck_round_device(field, t_tables, n_vars, r_prev=None, stream=None):
    """sumcheck_round() on device-resident torch tensors; with r_prev they are bound in place."""
    out = np.zeros((len(t_tables) + 1, 4), np.uint64)
    keep, rp = _opt(r_prev)
    check(L.lib().lw_sumcheck_round_device(field.field, _ptrs([t.data_ptr() for t in t_tables]), len(t_tables), n_vars, rp, L.host_ptr(out),
                                           L.stream_ptr(stream)))
    return out


def _add(field, a, b):
    """a + b of two stored elements (addition is the same in Montgomery form)"""
    to_int = lambda x: int.from_bytes(np.ascontiguousarray(x, dtype=np.uint64).astype(">u8").tobytes(), "big")
    s = (to_int(a) + to_int(b)) % MODULI[field.field]
    return np.frombuffer(s.to_bytes(32, "big"), dtype=">u8").astype(np.uint64)


def _prove_device(field, round_fn, t_finish, n_vars, challenge, stream):
    """The prover's loop: round_fn(n, r_prev) for one plain round and n_vars - 1 fused rounds (bind the previous challenge,
    then sum), then fix_variables of the last variable of every tensor of t_finish.
    -> (claimed_sum (4,), rounds, point (n_vars, 4), final_evals (len(t_finish), 4))"""
    import torch
    rounds, point = [], []
    r = None
    for i in range(n_vars):
        g = round_fn(n_vars - max(0, i - 1), r)
        rounds.append(g)
        r = np.ascontiguousarray(challenge(g), dtype=np.uint64).reshape(-1)[:4].copy()
        point.append(r)
    claimed = _add(field, rounds[0][0], rounds[0][1])
    t_fin = torch.empty((len(t_finish), 4), dtype=torch.int64, device=t_finish[0].device)
    for k, t in enumerate(t_finish):
        fix_variables_device(field, t, 1, r.reshape(1, 4), t_fin[k], stream)
    if stream is None:
        torch.cuda.current_stream().synchronize()
    else:
        torch.cuda.synchronize()
    final = t_fin.cpu().numpy().view(np.uint64)
    return claimed, rounds, np.stack(point), final


def sumcheck_prove_device(field, t_tables, n_vars, challenge, stream=None):
    """The prover's side of a sumcheck of prod_k t_tables[k] over the cube of n_vars >= 1 variables, the tables resident
    on the device and consumed in place.  challenge: a callable from a round's (K + 1, 4) array to the next r (4 uint64),
    the seam for the caller's transcript.  One plain round, n_vars - 1 fused rounds (bind the previous challenge, then
    sum), and a final fix_variables of the last variable.
    -> (claimed_sum (4,), rounds [n_vars arrays (K + 1, 4)], point (n_vars, 4), final_evals (K, 4))"""
    return _prove_device(field, lambda n, r: sumcheck_round_device(field, t_tables, n, r, stream), t_tables, n_vars, challenge, stream)


# ---- the table of eq(point, .) and the round over an eq-weighted sum of products ----
MAX_TERM_TABLES = 4
MAX_TERMS = 8
MAX_TERM_FACTORS = 3


def eq_table(field, point):
    """(2^n, 4): out[i] = prod_j eq(point[j], bit_{n-1-j}(i)) for a point of n coordinates, the reference's chis table."""
    n = len(point)
    p = _point(point, n)
    out = np.zeros((1 << n, 4), np.uint64)
    check(L.lib().lw_multilinear_eq_table(field.field, L.host_ptr(p), n, L.host_ptr(out)))
    return out


def eq_table_device(field, point, t_out=None, stream=None):
    """eq_table() into the device-resident tensor t_out (at least 2^n elements; a new (2^n, 4) int64 tensor when None);
    nothing is waited for.  -> t_out"""
    n = len(point)
    p = _point(point, n)
    if t_out is None:
        import torch
        t_out = torch.empty((1 << n, 4), dtype=torch.int64, device="cuda")
    if t_out.numel() * t_out.element_size() < 32 << n or not t_out.is_contiguous():
        from .errors import LengthMismatch
        raise LengthMismatch(f"the output holds fewer than 2^{n} contiguous elements")
    check(L.lib().lw_multilinear_eq_table_device(field.field, L.host_ptr(p), n, L.device_ptr(t_out), L.stream_ptr(stream)))
    return t_out


def _terms(field, terms, has_eq):
    """terms [(coeff or None, (table indices ...)), ...] -> (masks, coefficient array or None, D)"""
    from .errors import InputError
    masks = np.zeros(max(1, len(terms)), np.uint32)
    coeffs, deg = [], 0
    for t, (c, idx) in enumerate(terms):
        idx = [int(m) for m in idx]
        if len(set(idx)) != len(idx) or any(m < 0 or m >= 32 for m in idx):
            raise InputError(f"term {t}: every table at most once (no powers), indices from 0")
        masks[t] = sum(1 << m for m in idx)
        deg = max(deg, len(idx))
        coeffs.append(c)
    carr = None
    if any(c is not None for c in coeffs):
        one = np.frombuffer(((1 << 256) % MODULI[field.field]).to_bytes(32, "big"), dtype=">u8").astype(np.uint64)
        carr = np.stack([one if c is None else np.ascontiguousarray(c, dtype=np.uint64).reshape(-1)[:4] for c in coeffs])
        carr = np.ascontiguousarray(carr)
    return masks, carr, deg + (1 if has_eq else 0)


def sumcheck_terms_round(field, tables, terms, eq=None, r_prev=None):
    """(D + 1, 4): g(0) .. g(D) of the round of sum_x E(x) sum_t c_t prod_{m in S_t} T_m(x) over at most 4 tables of 2^n
    elements.  terms: a list of (coeff_or_None, (table indices ...)), at most 8, each over at most 3 distinct tables; None
    is the coefficient one.  eq: the table E or None.  D = the most tables in a term, plus one with eq.  With r_prev the
    tables and eq (which must then be writable (2^n, 4) uint64 arrays) are first bound to it in place, as in
    sumcheck_round."""
    every = list(tables) + ([eq] if eq is not None else [])
    ts = [_elems(t) for t in every]
    _bound_in_place(r_prev, every)
    n = _n_vars(ts[0]) if ts else 0
    masks, carr, deg = _terms(field, terms, eq is not None)
    out = np.zeros((deg + 1, 4), np.uint64)
    keep, rp = _opt(r_prev)
    k = len(tables)
    check(L.lib().lw_sumcheck_terms_round(field.field, _ptrs([t.ctypes.data for t in ts[:k]]), k,
                                          C.c_void_p(ts[k].ctypes.data) if eq is not None else None,   # an eq given stays one, even empty
                                          L.host_ptr(masks), L.host_ptr(carr), len(terms), n, rp, L.host_ptr(out)))
    return out


def sumcheck_terms_round_device(field, t_tables, terms, n_vars, t_eq=None, r_prev=None, stream=None):
    """sumcheck_terms_round() on device-resident torch tensors; with r_prev they are bound in place."""
    masks, carr, deg = _terms(field, terms, t_eq is not None)
    for t in list(t_tables) + ([t_eq] if t_eq is not None else []):
        if 0 <= n_vars <= 30 and t.numel() * t.element_size() < 32 << n_vars:
            from .errors import LengthMismatch
            raise LengthMismatch(f"a table holds fewer than 2^{n_vars} elements")
    out = np.zeros((deg + 1, 4), np.uint64)
    keep, rp = _opt(r_prev)
    check(L.lib().lw_sumcheck_terms_round_device(field.field, _ptrs([t.data_ptr() for t in t_tables]), len(t_tables),
                                                 L.device_ptr(t_eq) if t_eq is not None else None, L.host_ptr(masks), L.host_ptr(carr),
                                                 len(terms), n_vars, rp, L.host_ptr(out), L.stream_ptr(stream)))
    return out


def sumcheck_terms_prove_device(field, t_tables, terms, n_vars, challenge, t_eq=None, stream=None):
    """The prover's side of a sumcheck of sum_x E(x) sum_t c_t prod_{m in S_t} T_m(x) over the cube of n_vars >= 1
    variables, the tables and t_eq resident on the device and consumed in place.  challenge: a callable from a round's
    (D + 1, 4) array to the next r (4 uint64), the seam for the caller's transcript.  The loop of sumcheck_prove_device: one
    plain round, n_vars - 1 fused rounds, and a final fix_variables of the last variable.
    -> (claimed_sum (4,), rounds [n_vars arrays (D + 1, 4)], point (n_vars, 4), final_evals (K, 4) or (K + 1, 4) with
    the eq table's value last)"""
    every = list(t_tables) + ([t_eq] if t_eq is not None else [])
    return _prove_device(field, lambda n, r: sumcheck_terms_round_device(field, t_tables, terms, n, t_eq, r, stream), every, n_vars,
                         challenge, stream)
