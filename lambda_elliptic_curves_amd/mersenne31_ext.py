"""The quartic extension of Mersenne31, QM31 = CM31[u] / (u^2 - (2 + i)) over CM31 = F_p[i] / (i^2 + 1)
(Degree4ExtensionField / Degree2ExtensionField of the reference's mersenne31/extensions.rs), and the steps a circle STARK
prover runs in it on device-resident data: out-of-domain evaluation in the basis of the circle FFT, the DEEP quotients by
the lines through a point and its conjugate, and the circle FRI commit phase in evaluation form with Monolith layer trees.

A word is one uint32 as in circle.py: any word is accepted and read as (w & p) + (w >> 31), every word handed back is the
canonical residue.  A host-side scalar is a tuple (c0, c1, c2, c3) = (c0 + c1 i) + (c2 + c3 i) u; a point is (X, Y), two
scalars.  A vector of n elements on the device is a torch int32 tensor of four PLANES of n words, c0, then c1 `stride` words
later, and so on (0: dense): the same bytes circle.lde_device takes as batch = 4 and monolith.commit_columns_device as
n_cols = 4.  The domain is the standard coset in natural order, as circle.py has it.  Everything runs on torch's current
stream unless `stream` is given.
"""
import numpy as np

from . import _lib as L
from . import _ext_common as X
from ._ext_common import scalars
from .errors import InputError, check

P = (1 << 31) - 1
MUL, SQR, INV, MUL_BASE = L.M31EXT4_MUL, L.M31EXT4_SQR, L.M31EXT4_INV, L.M31EXT4_MUL_BASE
MAX_LOG = 30


def _scalars(values, count):
    """`count` scalars [(c0, c1, c2, c3), ...] -> a (count, 4) uint32 array; any u32 is a word"""
    return scalars(values, count, 4, np.uint32, 0xFFFFFFFF)


def _points(points):
    """[(X, Y), ...] -> a (m, 8) uint32 array"""
    return _scalars([c for pt in points for c in pt], 2 * len(points)).reshape(-1, 8)


def _word(w):
    w = int(w) & 0xFFFFFFFF
    return ((w & P) + (w >> 31)) % P


# ---- host-side helpers
def times_i(a):
    """(c0, c1, c2, c3) -> i (c0, c1, c2, c3)"""
    a = [_word(c) for c in a]
    return (-a[1] % P, a[0], -a[3] % P, a[2])


def times_u(a):
    """(A0 + A1 u) u = (2 + i) A1 + A0 u"""
    a = [_word(c) for c in a]
    return ((2 * a[2] - a[3]) % P, (2 * a[3] + a[2]) % P, a[0], a[1])


def combine_planes(v):
    """The value v[0] + i v[1] + u v[2] + i u v[3] of a polynomial with QM31 coefficients from the values of its four planes."""
    parts = [tuple(_word(c) for c in v[0]), times_i(v[1]), times_u(v[2]), times_i(times_u(v[3]))]
    return tuple(sum(p[e] for p in parts) % P for e in range(4))


def plane_weights(w):
    """The four weight rows of a QM31 column passed as its four planes: [w, i w, u w, i u w] for each weight of the row."""
    return [[tuple(_word(c) for c in e) for e in w], [times_i(e) for e in w], [times_u(e) for e in w], [times_i(times_u(e)) for e in w]]


# ---- the calls
def pointwise_device(op, t_a, t_b, t_out, n, a_stride=0, b_stride=0, out_stride=0, stream=None):
    """t_out[i] = t_a[i] t_b[i] (MUL), t_a[i]^2 (SQR), t_a[i]^-1 (INV; the inverse of 0 is 0) or t_a[i] t_b[i] with t_b a
    single plane of base-field words (MUL_BASE), for n elements.  t_b may be None for SQR and INV; t_out may be t_a or t_b."""
    check(L.lib().lw_mersenne31_ext4_pointwise_device(op, L.device_ptr(t_a), a_stride, L.device_ptr(t_b) if t_b is not None else None, b_stride,
                                                     L.device_ptr(t_out), out_stride, n, L.stream_ptr(stream)))
    return t_out


def evaluate_device(t_coeffs, n_cols, log2n, points, col_stride=0, stream=None):
    """Out-of-domain evaluation: n_cols columns of 2^log2n base-field coefficients in the basis of circle.evaluate_cfft
    (col_stride apart) at the `points` [(X, Y), ...] of QM31^2, which need not lie on the circle -> an (n_cols, m, 4) uint32
    array.  Waits for the stream."""
    pts = _points(points)
    out = np.zeros((n_cols, len(points), 4), np.uint32)
    check(L.lib().lw_mersenne31_ext4_evaluate_device(L.device_ptr(t_coeffs), n_cols, col_stride, log2n, L.host_ptr(pts), len(points), L.host_ptr(out),
                                                    L.stream_ptr(stream)))
    return out


def evaluate_ext_device(t_coeffs, log2n, points, plane_stride=0, stream=None):
    """A polynomial with QM31 coefficients (four planes) at the points -> [(c0, c1, c2, c3), ...]."""
    v = evaluate_device(t_coeffs, 4, log2n, points, plane_stride, stream)
    return [combine_planes(v[:, j]) for j in range(len(points))]


def deep_quotients_device(t_lde, n_cols, log2n, points, weights, evals, t_out, col_stride=0, out_stride=0, stream=None):
    """t_out[i] = sum_j (sum_k weights[k][j] (c_j col_k[i] - a_kj y_i - b_kj)) / D_j(x_i, y_i) over the 2^log2n points of the
    standard coset, the quotients by the lines through points[j] = (X_j, Y_j) and its conjugate (c, a, b and D as
    lw_hip.h states them; evals[k][j] is the claimed value of column k at point j).  weights, evals: n_cols rows of m
    scalars; t_out: a vector of 2^log2n elements.  A QM31 column is its four planes as four columns with the weight rows of
    plane_weights().  A point that is its own conjugate is refused."""
    m = len(points)
    pts, w, e = _points(points), _scalars([x for row in weights for x in row], n_cols * m), _scalars([x for row in evals for x in row], n_cols * m)
    check(L.lib().lw_mersenne31_ext4_deep_quotients_device(L.device_ptr(t_lde), n_cols, col_stride, log2n, L.host_ptr(pts), m, L.host_ptr(w), L.host_ptr(e),
                                                          L.device_ptr(t_out), out_stride, L.stream_ptr(stream)))
    return t_out


def fri_fold_device(t_evals, log2m, zeta, first, t_out=None, in_stride=0, out_stride=0, stream=None):
    """One circle FRI fold in evaluation form: t_out[i] = (v[i] + v[M-1-i] + zeta (v[i] - v[M-1-i]) / t_i) / 2 for i < M / 2,
    M = 2^log2m, with t_i = y_i of the coset of size M for the first fold (circle to line) and x_i of the coset of size 2M
    for every later one.  Enqueues and returns t_out (default: a new dense vector of M / 2 elements)."""
    import torch
    if t_out is None:
        t_out = torch.empty(4 * max((1 << log2m) // 2, 1), dtype=torch.int32, device=t_evals.device)
    z = _scalars([zeta], 1)
    check(L.lib().lw_mersenne31_ext4_fri_layer_device(L.device_ptr(t_evals), in_stride, log2m, L.host_ptr(z), 1 if first else 0, L.device_ptr(t_out), out_stride,
                                                     0, None, None, None, L.stream_ptr(stream)))
    return t_out


def fri_layer_device(t_evals, log2m, zeta, first, rounds, in_stride=0, stream=None):
    """A fold and the commitment of its result: the M / 2 folded values (at least 4) under a Monolith tree with M / 4
    leaves, leaf i the hash of (v'[i].c0..c3, v'[M/2-1-i].c0..c3), that is monolith.commit_columns(rounds, the eight pair
    columns, bit_reverse=False).  -> (t_folded: four dense planes of M / 2 words, t_nodes: (M / 2 - 1) x 8 int32, root first,
    readable by merkle.open_trees_device, root: (8,) uint32).  Waits for the stream."""
    import torch
    half = (1 << log2m) // 2
    t_out = torch.empty(4 * max(half, 1), dtype=torch.int32, device=t_evals.device)
    t_pairs = torch.empty(max(4 * half, 4), dtype=torch.int32, device=t_evals.device)   # 8 columns of half / 2 words, read by the tree only; the root's download waits for it
    t_nodes = torch.empty((max(half - 1, 1), 8), dtype=torch.int32, device=t_evals.device)
    z, root = _scalars([zeta], 1), np.zeros(8, np.uint32)
    check(L.lib().lw_mersenne31_ext4_fri_layer_device(L.device_ptr(t_evals), in_stride, log2m, L.host_ptr(z), 1 if first else 0, L.device_ptr(t_out), 0,
                                                     rounds, L.device_ptr(t_pairs), L.device_ptr(t_nodes), L.host_ptr(root), L.stream_ptr(stream)))
    return t_out, t_nodes, root


def fri_commit_phase_device(t_evals, log2n, number_layers, rounds, challenge, in_stride=0, stream=None):
    """The commit phase of circle FRI on a resident vector of 2^log2n evaluations: number_layers folds, fold k with
    zeta_k = challenge(root of the layer committed just before, or None); every folded layer but the last is committed.
    -> (last layer: [(c0, c1, c2, c3)] * (2^log2n >> number_layers), [(t_evals, t_nodes, root), ...]), the layers left on the
    device.  A number_layers that would commit a layer of fewer than 4 values or fold a single value is refused."""
    log2n, number_layers = int(log2n), int(number_layers)
    if not 1 <= log2n <= MAX_LOG:
        raise InputError(f"mersenne31_ext: a domain of 2^{log2n} points")
    if number_layers < 1 or number_layers > log2n or (number_layers >= 2 and log2n - (number_layers - 1) < 2):
        raise InputError(f"mersenne31_ext: {number_layers} layers from 2^{log2n} values: a committed layer has at least 4 values, a fold at least 2")
    layers, prev, t_cur, stride = [], None, t_evals, in_stride
    for k in range(number_layers):
        lg = log2n - k
        if k + 1 < number_layers:
            t_cur, t_nodes, prev = fri_layer_device(t_cur, lg, challenge(prev), k == 0, rounds, in_stride=stride, stream=stream)
            layers.append((t_cur, t_nodes, prev))
        else:
            t_cur = fri_fold_device(t_cur, lg, challenge(prev), k == 0, in_stride=stride, stream=stream)
        stride = 0
    count = 1 << (log2n - number_layers)
    last = t_cur.cpu().numpy().view(np.uint32).reshape(4, count)
    return [tuple(int(last[e, i]) for e in range(4)) for i in range(count)], layers


# ---- round 2: the composition polynomial on the circle
def _mul(a, b):
    """the product of two scalars (canonical words)"""
    a0, a1, a2, a3 = a
    b0, b1, b2, b3 = b
    t0, t1 = (a2 * b2 - a3 * b3) % P, (a2 * b3 + a3 * b2) % P          # A1 B1, then (2 + i) A1 B1
    return ((a0 * b0 - a1 * b1 + 2 * t0 - t1) % P, (a0 * b1 + a1 * b0 + 2 * t1 + t0) % P,
            (a0 * b2 - a1 * b3 + a2 * b0 - a3 * b1) % P, (a0 * b3 + a1 * b2 + a2 * b1 + a3 * b0) % P)


def part_factors(point, log2_part, n_parts):
    """The factors M_j(X) of H(z) = sum_j M_j(z.x) H_j(z) for the parts of composition_parts_device at the point z = (X, Y):
    M_j = prod_{t: bit t of j set} pi^(log2_part + t - 1)(X), pi(x) = 2 x^2 - 1 -> n_parts scalars."""
    log2_part, n_parts = int(log2_part), int(n_parts)
    if log2_part < 1 or n_parts < 1 or n_parts & (n_parts - 1):
        raise InputError(f"mersenne31_ext: {n_parts} parts of 2^{log2_part} coefficients")
    f = tuple(_word(c) for c in point[0])
    for _ in range(log2_part - 1):
        s = _mul(f, f)
        f = ((2 * s[0] - 1) % P, 2 * s[1] % P, 2 * s[2] % P, 2 * s[3] % P)
    out = [(1, 0, 0, 0)]
    while len(out) < n_parts:          # f = pi^(log2_part + t - 1)(X) doubles the list at bit t
        out += [_mul(m, f) for m in out]
        s = _mul(f, f)
        f = ((2 * s[0] - 1) % P, 2 * s[1] % P, 2 * s[2] % P, 2 * s[3] % P)
    return out


_R2 = X.Round2Spec(4, np.uint32, "int32", _scalars, None, L.M31qBoundary, L.M31qTransition, "lw_mersenne31_ext4_constraint_evaluations_device",
                   "lw_mersenne31_ext4_composition_parts_device", False)


def constraint_evaluations_device(program, consts, t_columns, log2_trace, log2_blowup, boundary, transitions, t_out=None, out_stride=0, col_log2_len=None,
                                  stream=None):
    """The evaluations of the composition polynomial on the LDE coset q_i = g_2N + i g_N in one pass over the columns, no
    row of transition evaluations stored: t_out[i] = sum_c coeff_c T_c(i) E_c(q_i) / Z_c(q_i) + sum_k coeff_k (col_k[i] -
    value_k) (1 + x'_k) / y'_k with (x'_k, y'_k) = q_i - p_step_k, a vector of N = 2^(log2_trace + log2_blowup) elements (Z, E
    as lw_hip.h states them).  program: stark.compile_transitions(...) with base-field constants `consts`; t_columns: a list
    of resident columns of N words (2^col_log2_len[c] for a short one); boundary: [(col, step, value, (c0, c1, c2, c3))];
    transitions: [dict(period, offset, end_exemptions, coeff=(c0, c1, c2, c3))].  Enqueues and returns t_out."""
    return X.constraint_evaluations(_R2, program, consts, t_columns, log2_trace, log2_blowup, boundary, transitions, t_out, out_stride, None, 0,
                                    col_log2_len, stream)


def composition_parts_device(t_evals, log2_lde, log2_part, n_parts, evals_stride=0, lde=True, tail=False, stream=None):
    """interpolate_cfft of the four planes and the parts of the result: part j is the block of coefficients
    [j L, (j + 1) L), L = 2^log2_part, and H(z) = sum_j part_factors(z, log2_part, n_parts)[j] H_j(z).
    -> (t_parts_coeffs: 4 P dense planes of L words, part j plane e at plane 4 j + e; t_parts_lde: 4 P dense planes of N words,
    every part on the LDE coset, or None; the number of non-zero words at the coefficient indices from P L on, or None with
    tail=False: nothing is waited for)."""
    import ctypes as C
    import torch
    P_, n_lde = max(int(n_parts), 1), 1 << int(log2_lde)
    t_coeffs = torch.empty(4 * P_ << max(int(log2_part), 0), dtype=t_evals.dtype, device=t_evals.device)
    t_lde = torch.empty(4 * P_ * n_lde, dtype=t_evals.dtype, device=t_evals.device) if lde else None
    count = C.c_uint64(0)
    check(L.lib().lw_mersenne31_ext4_composition_parts_device(L.device_ptr(t_evals), int(evals_stride), int(log2_lde), int(log2_part), int(n_parts),
                                                             L.device_ptr(t_coeffs), L.device_ptr(t_lde) if lde else None, C.byref(count) if tail else None,
                                                             L.stream_ptr(stream)))
    return t_coeffs, t_lde, (int(count.value) if tail else None)


def round2_device(program, consts, t_columns, log2_trace, log2_blowup, boundary, transitions, log2_part, n_parts, rounds, col_log2_len=None, stream=None):
    """Round 2 on resident LDE columns: the constraint evaluations, the parts and the Monolith column commitment over the 4 P
    planes of the parts on the LDE coset (monolith.commit_columns_device, bit-reversed rows).
    -> (t_parts_coeffs, t_parts_lde, t_nodes: (2 N - 1) x 8 int32, root: (8,) uint32).  Waits for the stream."""
    import torch
    from . import monolith
    log2_lde = int(log2_trace) + int(log2_blowup)
    t_ev = constraint_evaluations_device(program, consts, t_columns, log2_trace, log2_blowup, boundary, transitions, col_log2_len=col_log2_len, stream=stream)
    t_coeffs, t_lde, _ = composition_parts_device(t_ev, log2_lde, log2_part, n_parts, stream=stream)
    t_nodes = torch.empty((2 * (1 << log2_lde) - 1, 8), dtype=torch.int32, device=t_ev.device)
    root = monolith.commit_columns_device(int(rounds), t_lde, 4 * int(n_parts), log2_lde, t_nodes, stream=stream)
    return t_coeffs, t_lde, t_nodes, root
