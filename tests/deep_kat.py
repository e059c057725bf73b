"""Python big-integer restatement of the STARK prover's DEEP composition polynomial (compute_deep_composition_poly and
compute_trace_term, provers/stark/src/prover.rs:643-714, 720-747, with the gamma split of :559-572), term by term as the
reference writes it: subtract the evaluation, Ruffini-divide each term, scale, add, strip.  Values are canonical integers
mod p; the helpers at the bottom move between them and the stored (Montgomery) arrays the library takes.

horner and ruffini are tests/plonk_kat_round45.py's; its padd and pscale are fixed to the BLS12-381 scalar field, so the two
are restated here over any modulus."""
import numpy as np

from tests import plonk_kat_round45 as K

horner, ruffini = K.horner, K.ruffini


def padd(p, *ps):
    out = [0] * max((len(a) for a in ps), default=0)
    for a in ps:
        for i, c in enumerate(a):
            out[i] = (out[i] + c) % p
    return out


def pscale(a, s, p):
    return [c * s % p for c in a]


def strip(a):
    n = len(a)
    while n and a[n - 1] == 0:
        n -= 1
    return a[:n]


def sub_const(a, y, p):
    """Polynomial - FieldElement; the zero polynomial evaluates to 0 and stays zero"""
    if not a:
        return []
    return [(a[0] - y) % p] + list(a[1:])


def gammas(gamma, n_trace_polys, n_frame_rows, n_parts, p):
    """(trace_term_coeffs [C][T], composition gammas [P]): successors of 1 under * gamma, drained as prover.rs:559-572"""
    pw, g = [], 1
    for _ in range(n_trace_polys * n_frame_rows + n_parts):
        pw.append(g)
        g = g * gamma % p
    nt = n_trace_polys * n_frame_rows
    return [pw[j * n_frame_rows:(j + 1) * n_frame_rows] for j in range(n_trace_polys)], pw[nt:]


def deep_literal(trace_polys, parts, z, g, n_frame_rows, gamma, p):
    """compute_deep_composition_poly; -> the stripped coefficient list"""
    tw, hw = gammas(gamma, len(trace_polys), n_frame_rows, len(parts), p)
    z_power = pow(z, len(parts), p)
    h_terms = []
    for i, part in enumerate(parts):
        h_i_eval = horner(part, z_power, p)
        h_terms = padd(p, h_terms, pscale(sub_const(part, h_i_eval, p), hw[i], p))
    assert horner(h_terms, z_power, p) == 0
    h_terms, _ = ruffini(h_terms, z_power, p)
    trace_terms = []
    for j, t_j in enumerate(trace_polys):
        trace_int = []
        for offset in range(n_frame_rows):
            z_shifted = pow(g, offset, p) * z % p
            poly = sub_const(t_j, horner(t_j, z_shifted, p), p)
            poly, _ = ruffini(poly, z_shifted, p)
            trace_int = padd(p, trace_int, pscale(poly, tw[j][offset], p))
        trace_terms = padd(p, trace_terms, trace_int)
    return strip(padd(p, h_terms, trace_terms))


def deep_terms_literal(polys, points, weights, p):
    """sum_k sum_j weights[k][j] * quot(polys[k] - polys[k](points[j]), points[j]), one term after the other; zero weights
    contribute nothing.  -> the coefficient list padded to the longest length - 1 (not stripped)."""
    n = max((len(a) for a in polys), default=0)
    acc = [0] * max(0, n - 1)
    for a, row in zip(polys, weights):
        for x, w in zip(points, row):
            if w == 0:
                continue
            q, _ = ruffini(sub_const(a, horner(a, x, p), p), x, p)
            acc = padd(p, acc, pscale(q, w, p))
    return acc


def deep_formula(polys, points, weights, p):
    """sum_j quot(sum_k weights[k][j] polys[k], points[j]): what the library computes; padded like deep_terms_literal"""
    n = max((len(a) for a in polys), default=0)
    acc = [0] * max(0, n - 1)
    for j, x in enumerate(points):
        comb = padd(p, [0] * n, *[pscale(a, row[j], p) for a, row in zip(polys, weights)])
        q, _ = ruffini(comb, x, p)
        acc = padd(p, acc, q)
    return acc


# ---- stored form ----
def to_ints(a):
    a = np.ascontiguousarray(a, dtype=np.uint64).reshape(-1, 4)
    b = a.astype(">u8").tobytes()
    return [int.from_bytes(b[32 * i:32 * i + 32], "big") for i in range(a.shape[0])]


def to_arr(vals):
    if not len(vals):
        return np.zeros((0, 4), np.uint64)
    b = b"".join(int(v).to_bytes(32, "big") for v in vals)
    return np.frombuffer(b, dtype=">u8").astype(np.uint64).reshape(-1, 4)


def rinv(p):
    return pow(1 << 256, -1, p)


def unmont(a, p):
    """stored array -> canonical integers"""
    ri = rinv(p)
    return [v * ri % p for v in to_ints(a)]


def mont(vals, p):
    """canonical integers -> stored array"""
    return to_arr([v * (1 << 256) % p for v in vals])
