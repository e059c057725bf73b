"""The quartic extension of BabyBear, Fp4 = F_p[x] / (x^4 + 11) (Degree4BabyBearExtensionField of the reference, RISC Zero's
extension), and the prover steps that run in it on device-resident data: out-of-domain evaluation, the DEEP composition in
evaluation form and the FRI commit phase (fri::commit_phase<F, E> with F BabyBear, E = Fp4).

A word is a STORED BabyBear element: the Montgomery value a 2^32 mod p in a u32, below p (fft.Babybear31PrimeFieldU32's
layout); to_mont / from_mont go between integers and words.  A host-side Fp4 scalar is a tuple (c0, c1, c2, c3) of words,
a = c0 + c1 x + c2 x^2 + c3 x^3.  A vector of n elements on the device is a torch int32 tensor of four PLANES of n words,
c0, then c1 `stride` words later, and so on (0: dense): the same bytes fft.ntt_device / fft.lde_device take as batch = 4
and merkle.commit_columns_layout_device as n_cols = 4 under Babybear31PrimeFieldU32, so they transform and commit an Fp4
vector as it is.  Everything runs on torch's current stream unless `stream` is given.
"""
import numpy as np

from . import _lib as L
from . import _ext_common as X
from ._ext_common import commit_phase, folded_block, part_block_len, scalars  # noqa: F401  (folded_block, part_block_len: this module's surface)
from .errors import check

P = 2013265921
BETA = 11   # x^4 = -BETA
MUL, SQR, INV, MUL_BASE = L.BB4_MUL, L.BB4_SQR, L.BB4_INV, L.BB4_MUL_BASE
_R = 1 << 32
_R_INV = pow(_R, -1, P)


def to_mont(v):
    """an integer -> its stored word v 2^32 mod p"""
    return int(v) % P * _R % P


def from_mont(w):
    """a stored word -> the integer it stands for"""
    return int(w) * _R_INV % P


def _scalars(values, count):
    """`count` Fp4 scalars [(c0, c1, c2, c3), ...] -> a (count, 4) uint32 array"""
    return scalars(values, count, 4, np.uint32)


def _offset_arg(offset):
    """a coset offset as one stored word, or None"""
    return None if offset is None else np.array([int(offset)], np.uint32)


# ---- host-side helpers (stored words in, stored words out: both maps are linear over F)
def times_x(a):
    """(c0, c1, c2, c3) -> x (c0, c1, c2, c3) = (-11 c3, c0, c1, c2)"""
    return (-BETA * int(a[3]) % P, int(a[0]), int(a[1]), int(a[2]))


def combine_planes(v):
    """The value sum_e x^e v[e] of a polynomial with Fp4 coefficients from the values v[0 .. 3] of its four planes."""
    total, shifted = [0, 0, 0, 0], [tuple(int(c) for c in e) for e in v]
    for e in range(4):
        w = shifted[e]
        for _ in range(e):
            w = times_x(w)
        total = [(t + c) % P for t, c in zip(total, w)]
    return tuple(total)


def plane_weights(w):
    """The four weight rows of an Fp4 column passed as its four planes: [w, x w, x^2 w, x^3 w] for each weight of the row."""
    rows = [[tuple(int(c) for c in e) for e in w]]
    for _ in range(3):
        rows.append([times_x(e) for e in rows[-1]])
    return rows


# ---- the calls
def pointwise_device(op, t_a, t_b, t_out, n, a_stride=0, b_stride=0, out_stride=0, stream=None):
    """t_out[i] = t_a[i] t_b[i] (MUL), t_a[i]^2 (SQR), t_a[i]^-1 (INV; the inverse of 0 is 0) or t_a[i] t_b[i] with t_b a
    single plane of base-field words (MUL_BASE), for n elements.  t_b may be None for SQR and INV; t_out may be t_a or t_b."""
    check(L.lib().lw_babybear_ext4_pointwise_device(op, L.device_ptr(t_a), a_stride, L.device_ptr(t_b) if t_b is not None else None, b_stride,
                                                   L.device_ptr(t_out), out_stride, n, L.stream_ptr(stream)))
    return t_out


def to_planes_device(t_interleaved, t_planes, n, plane_stride=0, stream=None):
    """n elements of fft.Degree4BabyBearExtensionField's layout (4 x u64 per element, R = 2^64) -> four planes of stored words"""
    check(L.lib().lw_babybear_ext4_convert_device(L.BB4_TO_PLANES, L.device_ptr(t_interleaved), L.device_ptr(t_planes), plane_stride, n,
                                                 L.stream_ptr(stream)))
    return t_planes


def to_interleaved_device(t_planes, t_interleaved, n, plane_stride=0, stream=None):
    """four planes of stored words -> n elements of fft.Degree4BabyBearExtensionField's layout"""
    check(L.lib().lw_babybear_ext4_convert_device(L.BB4_TO_INTERLEAVED, L.device_ptr(t_interleaved), L.device_ptr(t_planes), plane_stride, n,
                                                 L.stream_ptr(stream)))
    return t_interleaved


def evaluate_device(t_coeffs, n_cols, n_coeffs, points, col_stride=0, stream=None):
    """Out-of-domain evaluation: n_cols base-field coefficient columns of n_coeffs words (col_stride apart) at the Fp4
    `points` [(c0, c1, c2, c3), ...] -> an (n_cols, m, 4) uint32 array.  Waits for the stream."""
    pts = _scalars(points, len(points))
    out = np.zeros((n_cols, len(points), 4), np.uint32)
    check(L.lib().lw_babybear_ext4_evaluate_device(L.device_ptr(t_coeffs), n_cols, col_stride, n_coeffs, L.host_ptr(pts), len(points),
                                                  L.host_ptr(out), L.stream_ptr(stream)))
    return out


def evaluate_ext_device(t_coeffs, n_coeffs, points, plane_stride=0, stream=None):
    """A polynomial with Fp4 coefficients (four planes) at the Fp4 points -> [(c0, c1, c2, c3), ...]."""
    v = evaluate_device(t_coeffs, 4, n_coeffs, points, plane_stride, stream)
    return [combine_planes(v[:, j]) for j in range(len(points))]


def deep_quotients_device(t_lde, n_cols, log2n, points, weights, evals, t_out, col_stride=0, out_stride=0, offset=None, stream=None):
    """t_out[i] = sum_j (sum_k weights[k][j] (col_k[i] - evals[k][j])) / (x_i - points[j]) over the 2^log2n rows of the LDE
    domain x_i = offset w^i.  weights, evals: n_cols rows of m Fp4 scalars; t_out: an Fp4 vector of 2^log2n elements.  An Fp4
    column is its four planes as four columns with the weight rows of plane_weights()."""
    m = len(points)
    pts, w, e = _scalars(points, m), _scalars([x for row in weights for x in row], n_cols * m), _scalars([x for row in evals for x in row], n_cols * m)
    check(L.lib().lw_babybear_ext4_deep_quotients_device(L.device_ptr(t_lde), n_cols, col_stride, log2n, L.host_ptr(_offset_arg(offset)),
                                                        L.host_ptr(pts), m, L.host_ptr(w), L.host_ptr(e), L.device_ptr(t_out), out_stride,
                                                        L.stream_ptr(stream)))
    return t_out


def fri_layer_device(t_coeffs, n_coeffs, zeta, coset_offset, domain_size, coeff_stride=0, fold_only=False, stream=None):
    """One layer of the FRI commit phase over Fp4: fold t_coeffs (an Fp4 vector of n_coeffs elements) with the challenge
    zeta = (c0, c1, c2, c3), evaluate the result on the coset of `domain_size` points (already halved) with offset
    `coset_offset` (a stored word, already squared) and commit pairs of evaluations in a Keccak-256 tree.
    -> (t_poly, t_evaluation, t_nodes, root): the folded block (four dense planes of folded_block(n_coeffs) words), the
    evaluation (four dense planes of domain_size words), the (domain_size - 1) x 32 bytes of nodes and the root as 32 bytes;
    with fold_only the last three are None."""
    import torch
    z = _scalars([zeta], 1)
    t_poly = torch.empty(4 * folded_block(n_coeffs), dtype=torch.int32, device=t_coeffs.device)
    if fold_only:
        check(L.lib().lw_babybear_ext4_fri_layer_device(L.device_ptr(t_coeffs), coeff_stride, n_coeffs, L.host_ptr(z), None, 0, L.device_ptr(t_poly),
                                                       None, None, None, L.stream_ptr(stream)))
        return t_poly, None, None, None
    t_eval = torch.empty(4 * domain_size, dtype=torch.int32, device=t_coeffs.device)
    t_nodes = torch.empty((max(domain_size - 1, 1), 32), dtype=torch.uint8, device=t_coeffs.device)
    out_root = np.zeros(32, np.uint8)
    check(L.lib().lw_babybear_ext4_fri_layer_device(L.device_ptr(t_coeffs), coeff_stride, n_coeffs, L.host_ptr(z), L.host_ptr(_offset_arg(coset_offset)),
                                                   domain_size, L.device_ptr(t_poly), L.device_ptr(t_eval), L.device_ptr(t_nodes),
                                                   L.host_ptr(out_root), L.stream_ptr(stream)))
    return t_poly, t_eval, t_nodes, out_root


def fri_commit_phase_device(t_coeffs, n_coeffs, number_layers, coset_offset, domain_size, challenge, stream=None):
    """fri::commit_phase (provers/stark/src/fri/mod.rs:22-75) over Fp4 on a device-resident polynomial: t_coeffs is an Fp4
    vector of n_coeffs coefficients in dense planes, domain_size and coset_offset (a stored word) those of the LDE domain.
    challenge(prev_root_or_None) -> (c0, c1, c2, c3) is the caller's transcript: called once per fold with the root of the
    layer committed just before (None for the first), it absorbs that root and samples the next zeta.  number_layers - 1
    layers are committed, then one more fold gives the constant.
    -> (last_value (c0, c1, c2, c3), [(t_evaluation, t_nodes, root), ...]), the layers left on the device."""
    def layer(t_poly, n, zeta, h, domain, fold_only):
        return fri_layer_device(t_poly, n, zeta, h, domain, fold_only=fold_only, stream=stream)

    def square(h):
        return h * h % P * _R_INV % P   # the stored word of the squared offset

    return commit_phase(layer, square, 4, t_coeffs, n_coeffs, number_layers, int(coset_offset), domain_size, challenge)


# ---- round 2: the composition polynomial
_R2 = X.Round2Spec(4, np.uint32, "int32", _scalars, _offset_arg, L.Bb4Boundary, L.Bb4Transition, "lw_babybear_ext4_constraint_evaluations_device",
                   "lw_babybear_ext4_composition_parts_device", False)


def constraint_evaluations_device(program, consts, t_columns, log2_trace, log2_blowup, boundary, transitions, t_out=None, out_stride=0, offset=None,
                                  col_log2_len=None, stream=None):
    """The evaluations of the composition polynomial on the LDE coset in one pass over the columns, no T_c rows stored:
    t_out[i] = sum_c coeff_c Z_c[i] T_c(i) + sum_k coeff_k (col_k[i] - value_k) / (x_i - g^step_k), an Fp4 vector of
    N = 2^(log2_trace + log2_blowup) elements.  program: stark.compile_transitions(...) with base-field constants `consts`
    (stored words); t_columns: a list of resident columns of N stored words (2^col_log2_len[c] for a short one); boundary:
    [(col, step, value, (c0, c1, c2, c3))]; transitions: [dict(period, offset, end_exemptions, exemptions_period,
    periodic_exemptions_offset, coeff=(c0, c1, c2, c3))]; offset: a stored word.  Enqueues and returns t_out."""
    return X.constraint_evaluations(_R2, program, consts, t_columns, log2_trace, log2_blowup, boundary, transitions, t_out, out_stride, offset, 0,
                                    col_log2_len, stream)


def composition_parts_device(t_evals, log2_lde, n_parts, evals_stride=0, offset=None, lde=True, lens=True, stream=None):
    """interpolate_offset_fft of the four planes, break_in_parts and the LDE of every part.
    -> (t_parts_coeffs: 4 P dense planes of part_block_len(log2_lde, P) words, part j plane e at plane 4 j + e; part_lens
    (None with lens=False: nothing is waited for); t_parts_lde: 4 P dense planes of N words, or None)."""
    return X.composition_parts(_R2, t_evals, log2_lde, n_parts, evals_stride, offset, 0, lde, lens, stream)


def round2_device(program, consts, t_columns, log2_trace, log2_blowup, boundary, transitions, n_parts, offset=None, col_log2_len=None, stream=None):
    """Round 2 on resident LDE columns: the constraint evaluations, the parts and the Keccak column commitment over the 4 P
    planes of the parts' LDE (merkle.commit_columns_layout_device, bit-reversed rows).
    -> (t_parts_coeffs, part_lens, t_parts_lde, t_nodes, root)"""
    import torch
    from . import fft, merkle
    log2_lde = int(log2_trace) + int(log2_blowup)
    t_ev = constraint_evaluations_device(program, consts, t_columns, log2_trace, log2_blowup, boundary, transitions, offset=offset,
                                         col_log2_len=col_log2_len, stream=stream)
    t_coeffs, lens, t_lde = composition_parts_device(t_ev, log2_lde, n_parts, offset=offset, stream=stream)
    t_nodes = torch.empty((2 * (1 << log2_lde) - 1) * 32, dtype=torch.uint8, device=t_ev.device)
    commit_root = merkle.commit_columns_layout_device(fft.Babybear31PrimeFieldU32, t_lde, 4 * int(n_parts), log2_lde, t_nodes, stream=stream)
    return t_coeffs, lens, t_lde, t_nodes, commit_root


# ---- RAP: the auxiliary column of round 1 and the round 2 that reads it
PRODUCT, SUM = L.EXT_AUX_PRODUCT, L.EXT_AUX_SUM


def _rap_interpolate(t_in, t_out, log2n, batch, root, stream):
    from . import fft
    fft.ntt_device(fft.Babybear31PrimeFieldU32, t_in, t_out, log2n, inverse=True, batch=batch, stream=stream)


def _rap_lde(t_coeffs, log2_coeffs, t_out, log2n, batch, offset, root, stream):
    from . import fft
    fft.lde_device(fft.Babybear31PrimeFieldU32, t_coeffs, log2_coeffs, t_out, log2n, batch=batch, offset=_offset_arg(offset), stream=stream)


def _rap_commit(t_lde, n_cols, log2n, stream):
    import torch
    from . import fft, merkle
    t_nodes = torch.empty((2 * (1 << log2n) - 1) * 32, dtype=torch.uint8, device=t_lde.device)
    return t_nodes, merkle.commit_columns_layout_device(fft.Babybear31PrimeFieldU32, t_lde, n_cols, log2n, t_nodes, stream=stream)


_RAP = X.RapSpec(_R2, L.Bb4RapBoundary, "lw_babybear_ext4_rap_constraint_evaluations_device", "lw_babybear_ext4_aux_fractions_device", _rap_interpolate,
                 _rap_lde, _rap_commit)


def aux_fractions_device(t_columns, n, num, den, mode=PRODUCT, exclusive=False, t_out=None, out_stride=0, total=False, count_zeros=False, stream=None):
    """The auxiliary column of a randomized AIR: with f_i = (a_0 + sum_j a_j col_{s_j}[i]) / (b_0 + sum_j b_j col_{t_j}[i]) over
    the n rows of the base columns t_columns, the running product (PRODUCT) or sum (SUM) of the f_i, inclusive (out[i] takes
    f_i in) or exclusive (out[0] = 1 or 0).  num = (a_0, [(s_j, a_j), ...]) and den likewise, the scalars in Fp4 (stored
    words), at most 16 terms each.  -> (t_out: four planes of n words out_stride apart, t_total: the product or sum over all
    rows as four words on the device, or None).  With count_zeros the call waits and raises errors.FieldError (.zero_denominators: how many) if a denominator
    is zero; without it the call only enqueues and the output of such rows is unspecified."""
    return X.aux_fractions(_RAP, t_columns, n, num, den, mode, exclusive, t_out, out_stride, total, count_zeros, stream)


def rap_constraint_evaluations_device(program, consts, xconsts, t_columns, t_aux_columns, log2_trace, log2_blowup, boundary, transitions, t_out=None,
                                      out_stride=0, aux_stride=0, offset=None, col_log2_len=None, stream=None):
    """constraint_evaluations_device for a randomized AIR: the program may read auxiliary columns (stark.xcell) and constants
    of Fp4 (stark.xconst).  xconsts: [(c0, c1, c2, c3)]; t_aux_columns: a list of resident Fp4 columns, four planes of N
    stored words aux_stride apart each; boundary: [(col, step, value, coeff)] or [(col, step, value, coeff, is_aux)] with
    value a stored word or four.  Enqueues and returns t_out."""
    return X.rap_constraint_evaluations(_RAP, program, consts, xconsts, t_columns, t_aux_columns, log2_trace, log2_blowup, boundary, transitions, t_out,
                                        out_stride, aux_stride, offset, 0, col_log2_len, stream)


def round1_aux_device(t_columns, log2_trace, log2_blowup, num, den, mode=PRODUCT, exclusive=False, offset=None, count_zeros=False, stream=None):
    """The second half of round 1 on resident trace columns of 2^log2_trace stored words: the auxiliary column
    (aux_fractions_device), the interpolation of its four planes, their LDE (fft.lde_device with batch = 4) and the Keccak
    column commitment over them.  count_zeros: wait for the column and raise errors.FieldError (with .zero_denominators) if a denominator is zero.
    -> (t_aux, t_total, t_polys, t_lde, t_nodes, root)"""
    return X.round1_aux(_RAP, t_columns, log2_trace, log2_blowup, num, den, mode, exclusive, offset, 0, count_zeros, stream)


def round2_rap_device(program, consts, xconsts, t_columns, t_aux_columns, log2_trace, log2_blowup, boundary, transitions, n_parts, offset=None,
                      col_log2_len=None, stream=None):
    """round2_device with rap_constraint_evaluations_device in the place of constraint_evaluations_device.
    -> (t_parts_coeffs, part_lens, t_parts_lde, t_nodes, root)"""
    log2_lde = int(log2_trace) + int(log2_blowup)
    t_ev = rap_constraint_evaluations_device(program, consts, xconsts, t_columns, t_aux_columns, log2_trace, log2_blowup, boundary, transitions,
                                             offset=offset, col_log2_len=col_log2_len, stream=stream)
    t_coeffs, lens, t_lde = composition_parts_device(t_ev, log2_lde, n_parts, offset=offset, stream=stream)
    t_nodes, commit_root = _rap_commit(t_lde, 4 * int(n_parts), log2_lde, stream)
    return t_coeffs, lens, t_lde, t_nodes, commit_root
