"""The quadratic extension of Goldilocks, Fp2 = F_p[t] / (t^2 - 7) (Goldilocks64ExtensionField of the reference, Plonky2's
quadratic extension), and the prover steps that run in it on device-resident data: out-of-domain evaluation, the DEEP
composition in evaluation form and the FRI commit phase (fri::commit_phase<F, E> with F Goldilocks, E = Fp2).

A host-side Fp2 scalar is a pair (c0, c1) of integers, a = c0 + c1 t.  A vector of n elements on the device is a torch
int64 tensor of two PLANES of n words, c0 then c1 `stride` words later (0: dense): the same bytes lw_goldilocks_ntt_device
takes as batch = 2 and lw_rpo_commit_columns_device as n_cols = 2, so goldilocks.ntt_device / lde_device transform an Fp2
vector as it is.  Everything runs on torch's current stream unless `stream` is given.
"""
import numpy as np

from . import _lib as L
from . import _ext_common as X
from ._ext_common import commit_phase, folded_block, part_block_len, scalars  # noqa: F401  (folded_block, part_block_len: this module's surface)
from .errors import check
from .goldilocks import P, _offset_arg

NON_RESIDUE = 7
MUL, SQR, INV, MUL_BASE = L.GL2_MUL, L.GL2_SQR, L.GL2_INV, L.GL2_MUL_BASE
RPO_128, RPO_160 = L.RPO_128, L.RPO_160
_M64 = (1 << 64) - 1


def _scalars(values, count):
    """`count` Fp2 scalars [(c0, c1), ...] (or one pair when count is 1) -> a (count, 2) uint64 array"""
    return scalars(values, count, 2, np.uint64, _M64)


# ---- host-side helpers
def times_t(a):
    """(c0, c1) -> t (c0, c1) = (7 c1, c0): the weight of the c1 plane of an Fp2 column"""
    return (NON_RESIDUE * int(a[1]) % P, int(a[0]) % P)


def combine_planes(v0, v1):
    """The value v0 + t v1 of a polynomial with Fp2 coefficients from the values of its two planes."""
    t1 = times_t(v1)
    return ((int(v0[0]) + t1[0]) % P, (int(v0[1]) + t1[1]) % P)


def plane_weights(w):
    """The two weight rows of an Fp2 column passed as its two planes: [w, t w] for each weight of the row."""
    return [tuple(int(c) % P for c in x) for x in w], [times_t(x) for x in w]


# ---- the calls
def pointwise_device(op, t_a, t_b, t_out, n, a_stride=0, b_stride=0, out_stride=0, stream=None):
    """t_out[i] = t_a[i] t_b[i] (MUL), t_a[i]^2 (SQR), t_a[i]^-1 (INV; the inverse of 0 is 0) or t_a[i] t_b[i] with t_b a
    single plane of base-field words (MUL_BASE), for n elements.  t_b may be None for SQR and INV; t_out may be t_a or t_b."""
    check(L.lib().lw_goldilocks_ext2_pointwise_device(op, L.device_ptr(t_a), a_stride, L.device_ptr(t_b) if t_b is not None else None, b_stride,
                                                     L.device_ptr(t_out), out_stride, n, L.stream_ptr(stream)))
    return t_out


def evaluate_device(t_coeffs, n_cols, n_coeffs, points, col_stride=0, stream=None):
    """Out-of-domain evaluation: n_cols base-field coefficient columns of n_coeffs words (col_stride apart) at the Fp2
    `points` [(c0, c1), ...] -> an (n_cols, m, 2) uint64 array.  Waits for the stream."""
    pts = _scalars(points, len(points))
    out = np.zeros((n_cols, len(points), 2), np.uint64)
    check(L.lib().lw_goldilocks_ext2_evaluate_device(L.device_ptr(t_coeffs), n_cols, col_stride, n_coeffs, L.host_ptr(pts), len(points),
                                                    L.host_ptr(out), L.stream_ptr(stream)))
    return out


def evaluate_ext_device(t_coeffs, n_coeffs, points, plane_stride=0, stream=None):
    """A polynomial with Fp2 coefficients (two planes) at the Fp2 points -> [(c0, c1), ...]."""
    v = evaluate_device(t_coeffs, 2, n_coeffs, points, plane_stride, stream)
    return [combine_planes(v[0, j], v[1, j]) for j in range(len(points))]


def deep_quotients_device(t_lde, n_cols, log2n, points, weights, evals, t_out, col_stride=0, out_stride=0, offset=None, root=0, stream=None):
    """t_out[i] = sum_j (sum_k weights[k][j] (col_k[i] - evals[k][j])) / (x_i - points[j]) over the 2^log2n rows of the LDE
    domain x_i = offset w^i.  weights, evals: n_cols rows of m Fp2 scalars; t_out: an Fp2 vector of 2^log2n elements.  An Fp2
    column is its two planes as two columns with the weight rows of plane_weights()."""
    m = len(points)
    pts, w, e = _scalars(points, m), _scalars([x for row in weights for x in row], n_cols * m), _scalars([x for row in evals for x in row], n_cols * m)
    check(L.lib().lw_goldilocks_ext2_deep_quotients_device(L.device_ptr(t_lde), n_cols, col_stride, log2n, L.host_ptr(_offset_arg(offset)), root,
                                                          L.host_ptr(pts), m, L.host_ptr(w), L.host_ptr(e), L.device_ptr(t_out), out_stride,
                                                          L.stream_ptr(stream)))
    return t_out


def digest_words(level):
    return 4 if level == RPO_128 else 5


def fri_layer_device(t_coeffs, n_coeffs, zeta, coset_offset, domain_size, level=RPO_128, coeff_stride=0, root=0, fold_only=False, stream=None):
    """One layer of the FRI commit phase over Fp2: fold t_coeffs (an Fp2 vector of n_coeffs elements) with the challenge
    zeta = (c0, c1), evaluate the result on the coset of `domain_size` points (already halved) with offset `coset_offset`
    (already squared) and commit pairs of evaluations in an RPO tree.
    -> (t_poly, t_evaluation, t_nodes, root): the folded block (two dense planes of folded_block(n_coeffs) words), the
    evaluation (two dense planes of domain_size words), the (domain_size - 1) digests and the root as a uint64 array;
    with fold_only the last three are None."""
    import torch
    z = _scalars([zeta], 1)
    t_poly = torch.empty(2 * folded_block(n_coeffs), dtype=torch.int64, device=t_coeffs.device)
    if fold_only:
        check(L.lib().lw_goldilocks_ext2_fri_layer_device(L.device_ptr(t_coeffs), coeff_stride, n_coeffs, L.host_ptr(z), None, 0, root, level,
                                                         L.device_ptr(t_poly), None, None, None, L.stream_ptr(stream)))
        return t_poly, None, None, None
    d = digest_words(level)
    t_eval = torch.empty(2 * domain_size, dtype=torch.int64, device=t_coeffs.device)
    t_nodes = torch.empty(max(domain_size - 1, 1) * d, dtype=torch.int64, device=t_coeffs.device)
    out_root = np.zeros(d, np.uint64)
    check(L.lib().lw_goldilocks_ext2_fri_layer_device(L.device_ptr(t_coeffs), coeff_stride, n_coeffs, L.host_ptr(z), L.host_ptr(_offset_arg(coset_offset)),
                                                     domain_size, root, level, L.device_ptr(t_poly), L.device_ptr(t_eval), L.device_ptr(t_nodes),
                                                     L.host_ptr(out_root), L.stream_ptr(stream)))
    return t_poly, t_eval, t_nodes, out_root


def fri_commit_phase_device(t_coeffs, n_coeffs, number_layers, coset_offset, domain_size, challenge, level=RPO_128, root=0, stream=None):
    """fri::commit_phase (provers/stark/src/fri/mod.rs:22-75) over Fp2 on a device-resident polynomial: t_coeffs is an Fp2
    vector of n_coeffs coefficients in dense planes, domain_size and coset_offset those of the LDE domain.
    challenge(prev_root_or_None) -> (c0, c1) is the caller's transcript: called once per fold with the root of the layer
    committed just before (None for the first), it absorbs that root and samples the next zeta.  number_layers - 1 layers
    are committed, then one more fold gives the constant.
    -> (last_value (c0, c1), [(t_evaluation, t_nodes, root), ...]), the layers left on the device."""
    def layer(t_poly, n, zeta, h, domain, fold_only):
        return fri_layer_device(t_poly, n, zeta, h, domain, level, root=root, fold_only=fold_only, stream=stream)

    def square(h):
        return h * h % P

    return commit_phase(layer, square, 2, t_coeffs, n_coeffs, number_layers, int(coset_offset) % P, domain_size, challenge)


# ---- round 2: the composition polynomial
_R2 = X.Round2Spec(2, np.uint64, "int64", _scalars, _offset_arg, L.Gl2Boundary, L.Gl2Transition, "lw_goldilocks_ext2_constraint_evaluations_device",
                   "lw_goldilocks_ext2_composition_parts_device", True)


def constraint_evaluations_device(program, consts, t_columns, log2_trace, log2_blowup, boundary, transitions, t_out=None, out_stride=0, offset=None,
                                  root=0, col_log2_len=None, stream=None):
    """The evaluations of the composition polynomial on the LDE coset in one pass over the columns, no T_c rows stored:
    t_out[i] = sum_c coeff_c Z_c[i] T_c(i) + sum_k coeff_k (col_k[i] - value_k) / (x_i - g^step_k), an Fp2 vector of
    N = 2^(log2_trace + log2_blowup) elements.  program: stark.compile_transitions(...) with base-field constants `consts`
    (integers); t_columns: a list of resident columns of N words (2^col_log2_len[c] for a short one); boundary:
    [(col, step, value, (c0, c1))]; transitions: [dict(period, offset, end_exemptions, exemptions_period,
    periodic_exemptions_offset, coeff=(c0, c1))].  Enqueues and returns t_out."""
    return X.constraint_evaluations(_R2, program, consts, t_columns, log2_trace, log2_blowup, boundary, transitions, t_out, out_stride, offset, root,
                                    col_log2_len, stream)


def composition_parts_device(t_evals, log2_lde, n_parts, evals_stride=0, offset=None, root=0, lde=True, lens=True, stream=None):
    """interpolate_offset_fft of the two planes, break_in_parts and the LDE of every part.
    -> (t_parts_coeffs: 2 P dense planes of part_block_len(log2_lde, P) words, part j plane e at plane 2 j + e; part_lens
    (None with lens=False: nothing is waited for); t_parts_lde: 2 P dense planes of N words, or None)."""
    return X.composition_parts(_R2, t_evals, log2_lde, n_parts, evals_stride, offset, root, lde, lens, stream)


def round2_device(program, consts, t_columns, log2_trace, log2_blowup, boundary, transitions, n_parts, offset=None, root=0, col_log2_len=None,
                  level=RPO_128, stream=None):
    """Round 2 on resident LDE columns: the constraint evaluations, the parts and the RPO column commitment over the 2 P
    planes of the parts' LDE (rpo.commit_columns_device, bit-reversed rows).
    -> (t_parts_coeffs, part_lens, t_parts_lde, t_nodes, root)"""
    import torch
    from . import rpo
    log2_lde = int(log2_trace) + int(log2_blowup)
    t_ev = constraint_evaluations_device(program, consts, t_columns, log2_trace, log2_blowup, boundary, transitions, offset=offset, root=root,
                                         col_log2_len=col_log2_len, stream=stream)
    t_coeffs, lens, t_lde = composition_parts_device(t_ev, log2_lde, n_parts, offset=offset, root=root, stream=stream)
    t_nodes = torch.empty((2 * (1 << log2_lde) - 1) * digest_words(level), dtype=torch.int64, device=t_ev.device)
    commit_root = rpo.commit_columns_device(level, t_lde, 2 * int(n_parts), log2_lde, t_nodes, stream=stream)
    return t_coeffs, lens, t_lde, t_nodes, commit_root


# ---- RAP: the auxiliary column of round 1 and the round 2 that reads it
PRODUCT, SUM = L.EXT_AUX_PRODUCT, L.EXT_AUX_SUM


def _rap_interpolate(t_in, t_out, log2n, batch, root, stream):
    from . import goldilocks
    goldilocks.ntt_device(t_in, t_out, log2n, inverse=True, batch=batch, root=root, stream=stream)


def _rap_lde(t_coeffs, log2_coeffs, t_out, log2n, batch, offset, root, stream):
    from . import goldilocks
    goldilocks.lde_device(t_coeffs, log2_coeffs, t_out, log2n, batch=batch, offset=offset, root=root, stream=stream)


def _rap_commit(level):
    def commit(t_lde, n_cols, log2n, stream):
        import torch
        from . import rpo
        t_nodes = torch.empty((2 * (1 << log2n) - 1) * digest_words(level), dtype=torch.int64, device=t_lde.device)
        return t_nodes, rpo.commit_columns_device(level, t_lde, n_cols, log2n, t_nodes, stream=stream)
    return commit


def _rap(level=RPO_128):
    return X.RapSpec(_R2, L.Gl2RapBoundary, "lw_goldilocks_ext2_rap_constraint_evaluations_device", "lw_goldilocks_ext2_aux_fractions_device",
                     _rap_interpolate, _rap_lde, _rap_commit(level))


def aux_fractions_device(t_columns, n, num, den, mode=PRODUCT, exclusive=False, t_out=None, out_stride=0, total=False, count_zeros=False, stream=None):
    """The auxiliary column of a randomized AIR: with f_i = (a_0 + sum_j a_j col_{s_j}[i]) / (b_0 + sum_j b_j col_{t_j}[i]) over
    the n rows of the base columns t_columns, the running product (PRODUCT) or sum (SUM) of the f_i, inclusive (out[i] takes
    f_i in) or exclusive (out[0] = 1 or 0).  num = (a_0, [(s_j, a_j), ...]) and den likewise, the scalars in Fp2, at most 16
    terms each.  -> (t_out: two planes of n words out_stride apart, t_total: the product or sum over all rows as two words on
    the device, or None).  With count_zeros the call waits and raises errors.FieldError (.zero_denominators: how many) if a denominator is zero; without it
    the call only enqueues and the output of such rows is unspecified."""
    return X.aux_fractions(_rap(), t_columns, n, num, den, mode, exclusive, t_out, out_stride, total, count_zeros, stream)


def rap_constraint_evaluations_device(program, consts, xconsts, t_columns, t_aux_columns, log2_trace, log2_blowup, boundary, transitions, t_out=None,
                                      out_stride=0, aux_stride=0, offset=None, root=0, col_log2_len=None, stream=None):
    """constraint_evaluations_device for a randomized AIR: the program may read auxiliary columns (stark.xcell) and constants
    of Fp2 (stark.xconst).  xconsts: [(c0, c1)]; t_aux_columns: a list of resident Fp2 columns, two planes of N words
    aux_stride apart each; boundary: [(col, step, value, (c0, c1))] or [(col, step, value, (c0, c1), is_aux)] with value a
    word or a pair.  Enqueues and returns t_out."""
    return X.rap_constraint_evaluations(_rap(), program, consts, xconsts, t_columns, t_aux_columns, log2_trace, log2_blowup, boundary, transitions, t_out,
                                        out_stride, aux_stride, offset, root, col_log2_len, stream)


def round1_aux_device(t_columns, log2_trace, log2_blowup, num, den, mode=PRODUCT, exclusive=False, offset=None, root=0, level=RPO_128, count_zeros=False,
                      stream=None):
    """The second half of round 1 on resident trace columns of 2^log2_trace words: the auxiliary column (aux_fractions_device),
    the interpolation of its two planes, their LDE (goldilocks.lde_device with batch = 2) and the RPO column commitment over
    them.  count_zeros: wait for the column and raise errors.FieldError (with .zero_denominators) if a denominator is zero.
    -> (t_aux, t_total, t_polys, t_lde, t_nodes, root)"""
    return X.round1_aux(_rap(level), t_columns, log2_trace, log2_blowup, num, den, mode, exclusive, offset, root, count_zeros, stream)


def round2_rap_device(program, consts, xconsts, t_columns, t_aux_columns, log2_trace, log2_blowup, boundary, transitions, n_parts, offset=None, root=0,
                      col_log2_len=None, level=RPO_128, stream=None):
    """round2_device with rap_constraint_evaluations_device in the place of constraint_evaluations_device.
    -> (t_parts_coeffs, part_lens, t_parts_lde, t_nodes, root)"""
    log2_lde = int(log2_trace) + int(log2_blowup)
    t_ev = rap_constraint_evaluations_device(program, consts, xconsts, t_columns, t_aux_columns, log2_trace, log2_blowup, boundary, transitions,
                                             offset=offset, root=root, col_log2_len=col_log2_len, stream=stream)
    t_coeffs, lens, t_lde = composition_parts_device(t_ev, log2_lde, n_parts, offset=offset, root=root, stream=stream)
    t_nodes, commit_root = _rap_commit(level)(t_lde, 2 * int(n_parts), log2_lde, stream)
    return t_coeffs, lens, t_lde, t_nodes, commit_root
