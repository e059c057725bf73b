"""The STARK prover's DEEP composition polynomial (compute_deep_composition_poly / compute_trace_term,
provers/stark/src/prover.rs:643-714, 720-747) on the device, between round 3 and fri::commit_phase (:575-594):

    deep = sum_i gamma'_i (H_i - H_i(z^P)) / (X - z^P)  +  sum_j sum_r gamma_{j,r} (t_j - y_{j,r}) / (X - g^r z)

over Stark252 or BLS12-381 Fr.  Elements are as stored (Montgomery form, 4 x uint64, MS limb first).  The evaluations the
reference subtracts are not taken: they change only coefficient 0, which no quotient coefficient reads.  Scalars (z, g,
gamma) are host values; their few products are done here in Python integers on the stored limbs."""
import numpy as np

from . import _lib as L
from . import poly

MODULI = {
    L.FIELD_STARK252: (1 << 251) + 17 * (1 << 192) + 1,
    L.FIELD_BLS12_381_FR: 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001,
}


def _int(e):
    w = np.ascontiguousarray(e, dtype=np.uint64).reshape(-1)[:4]
    return (int(w[0]) << 192) | (int(w[1]) << 128) | (int(w[2]) << 64) | int(w[3])


def _limbs(v):
    return [(v >> s) & 0xffffffffffffffff for s in (192, 128, 64, 0)]


def deep_terms(field, n_trace_polys, n_parts, n_frame_rows, z, primitive_root, gamma):
    """The points and the weight matrix of the DEEP composition polynomial, for lw_stark_deep_composition:
    polynomials t_0 .. t_{C-1}, H_0 .. H_{P-1} (K = C + P rows), points g^0 z .. g^(T-1) z, z^P (M = T + 1 columns),
    T = n_frame_rows = transition_offsets.len() * STEP_SIZE.
    Row r of the frame is divided at g^r z with r the enumeration index, as compute_trace_term does (prover.rs:739).
    Weights are the powers 1, gamma, gamma^2, ... in the reference's order (prover.rs:559-572): the first C * T go to the
    trace terms in runs of T per column, the next P to the composition parts; every other entry is zero.
    -> (points (M, 4), weights (K, M, 4)) uint64, stored form."""
    p = MODULI[field.field]
    r_inv = pow(1 << 256, -1, p)
    mul = lambda a, b: a * b * r_inv % p          # the product of two stored values, stored
    one = (1 << 256) % p
    Z, G, GA = _int(z), _int(primitive_root), _int(gamma)
    C_, P_, T = int(n_trace_polys), int(n_parts), int(n_frame_rows)
    pts, gr = [], one
    for _ in range(T):
        pts.append(mul(gr, Z))
        gr = mul(gr, G)
    zp = one
    for _ in range(P_):
        zp = mul(zp, Z)
    pts.append(zp)
    w = [[0] * (T + 1) for _ in range(C_ + P_)]
    g = one
    for j in range(C_):
        for r in range(T):
            w[j][r] = g
            g = mul(g, GA)
    for i in range(P_):
        w[C_ + i][T] = g
        g = mul(g, GA)
    points = np.array([_limbs(v) for v in pts], dtype=np.uint64).reshape(T + 1, 4)
    weights = np.array([[_limbs(v) for v in row] for row in w], dtype=np.uint64).reshape(C_ + P_, T + 1, 4)
    return points, weights


def deep_composition_poly_device(field, t_trace_polys, trace_lens, t_parts, part_lens, z, primitive_root, n_frame_rows, gamma,
                                 t_out, stream=None):
    """compute_deep_composition_poly on device-resident polynomials into t_out (longest length - 1 elements), which
    merkle.fri_commit_phase_device takes as it is.  -> (stripped length, trace values (C, T, 4) with [j, r] = t_j(g^r z),
    composition part values (P, 4) = H_i(z^P)): round 3's out-of-domain tables at the points the division uses."""
    C_, P_, T = len(t_trace_polys), len(t_parts), int(n_frame_rows)
    points, weights = deep_terms(field, C_, P_, T, z, primitive_root, gamma)
    n, ev = poly.deep_composition_device(field, list(t_trace_polys) + list(t_parts), list(trace_lens) + list(part_lens), points,
                                         weights, t_out, stream=stream)
    return n, ev[:C_, :T].copy(), ev[C_:, T].copy()
