"""What the extension-field modules (goldilocks_ext, babybear_ext) share on the host: the shape of their scalars, the
length of a folded block, the loop of the FRI commit phase and the calls of round 2 (constraint evaluations in one pass,
the parts of the composition polynomial)."""
import ctypes as C

import numpy as np


def scalars(values, count, width, dtype, mask=None):
    """`count` scalars of `width` words each [(c0, c1, ...), ...] -> a (count, width) array; with `mask` every word is
    taken modulo mask + 1"""
    word = int if mask is None else lambda c: int(c) & mask
    a = np.array([[word(c) for c in v] for v in values], dtype).reshape(-1, width) if count else np.zeros((0, width), dtype)
    if a.shape[0] != count:
        raise ValueError(f"{a.shape[0]} Fp{width} scalars where {count} are expected")
    return a


def folded_block(n_coeffs):
    """The length of the zero-padded block a fold of n_coeffs coefficients writes."""
    return max(2, 1 << max((n_coeffs + 1) // 2 - 1, 0).bit_length())


def commit_phase(layer, square, width, t_coeffs, n_coeffs, number_layers, coset_offset, domain_size, challenge):
    """fri::commit_phase (provers/stark/src/fri/mod.rs:22-75).  layer(t_poly, n, zeta, offset, domain_size, fold_only) is the
    module's fri_layer_device, square(h) the offset of the next layer's coset in the module's words.
    -> (the `width` words of the last value, [(t_evaluation, t_nodes, root), ...])"""
    layers, prev = [], None
    t_poly, n, h = t_coeffs, n_coeffs, coset_offset
    for _ in range(1, number_layers):
        domain_size //= 2
        h = square(h)
        t_poly, t_eval, t_nodes, layer_root = layer(t_poly, n, challenge(prev), h, domain_size, False)
        n = folded_block(n)   # the dense block, zero padding included, is the next layer's polynomial
        layers.append((t_eval, t_nodes, layer_root))
        prev = layer_root
    t_last, _, _, _ = layer(t_poly, n, challenge(prev), None, 0, True)
    block = t_last.numel() // width
    last = t_last.cpu().numpy().view(np.dtype(f"uint{8 * t_last.element_size()}"))
    return tuple(int(last[e * block]) for e in range(width)), layers


# ---- round 2: the composition polynomial (lw_*_constraint_evaluations_device, lw_*_composition_parts_device)
class Round2Spec:
    """What a module hands to the shared round-2 calls: the number of planes, the numpy and torch types of a word, its
    scalars(values, count), offset_arg(offset) (None: the calls take no coset offset, the domain is fixed), the ctypes
    entries of the two tables, the names of the two C calls and whether they take a two_adic_root."""

    def __init__(self, width, word, torch_word, scalars, offset_arg, boundary, transition, constraints, parts, rooted):
        self.width, self.word, self.torch_word, self.scalars, self.offset_arg = width, word, torch_word, scalars, offset_arg
        self.boundary, self.transition, self.constraints, self.parts, self.rooted = boundary, transition, constraints, parts, rooted


def part_block_len(log2_lde, n_parts):
    """next_power_of_two(ceil(N / P)): the zero-padded block a part of H is stored in."""
    per = -(-(1 << int(log2_lde)) // int(n_parts))
    return 1 << (per - 1).bit_length()


def _boundary_table(spec, boundary):
    """[(col, step, value, coeff)] -> the module's boundary array; value one word of F, coeff a scalar of E"""
    tab = (spec.boundary * max(1, len(boundary)))()
    for k, (col, step, value, coeff) in enumerate(boundary):
        tab[k].col, tab[k].step = int(col), int(step)
        tab[k].value = int(spec.scalars([(value,) * spec.width], 1)[0, 0])
        tab[k].coeff[:] = [int(x) for x in spec.scalars([coeff], 1)[0]]
    return tab


def _transition_table(spec, transitions):
    """[dict(period, offset, end_exemptions, exemptions_period (None / 0: none), periodic_exemptions_offset, coeff)] -> the
    module's transition array; coeff a scalar of E"""
    tab = (spec.transition * max(1, len(transitions)))()
    periodic = any(name == "exemptions_period" for name, _ in spec.transition._fields_)   # a circle zerofier has none
    for k, t in enumerate(transitions):
        tab[k].period, tab[k].offset = int(t.get("period", 1)), int(t.get("offset", 0))
        tab[k].end_exemptions = int(t.get("end_exemptions", 0))
        if periodic:
            tab[k].exemptions_period = int(t.get("exemptions_period") or 0)
            tab[k].periodic_exemptions_offset = int(t.get("periodic_exemptions_offset") or 0)
        elif t.get("exemptions_period"):
            raise ValueError("this extension's zerofiers have no exemptions_period")
        tab[k].coeff[:] = [int(x) for x in spec.scalars([t["coeff"]], 1)[0]]
    return tab


def constraint_evaluations(spec, program, consts, t_columns, log2_trace, log2_blowup, boundary, transitions, t_out, out_stride, offset, root,
                           col_log2_len, stream):
    from . import _lib as L
    from .errors import LengthMismatch, check
    from .stark import AIR_OP_DTYPE
    n_lde = 1 << (int(log2_trace) + int(log2_blowup))
    ops = np.ascontiguousarray(program.ops, dtype=AIR_OP_DTYPE)
    cs = spec.scalars([(c,) * spec.width for c in (consts if consts is not None else [])], len(consts) if consts is not None else 0)[:, 0].copy()
    if cs.shape[0] < program.n_consts:
        raise LengthMismatch(f"{cs.shape[0]} constants for a program that reads constant {program.n_consts - 1}")
    if len(t_columns) < program.n_cols:
        raise LengthMismatch(f"{len(t_columns)} columns for a program that reads column {program.n_cols - 1}")
    lens = None
    if col_log2_len is not None:
        lens = np.ascontiguousarray([int(x) for x in col_log2_len], dtype=np.uint32)
        if lens.shape[0] != len(t_columns):
            raise LengthMismatch(f"{lens.shape[0]} column lengths for {len(t_columns)} columns")
    if t_out is None:
        import torch
        t_out = torch.empty(spec.width * n_lde, dtype=getattr(torch, spec.torch_word), device=t_columns[0].device if len(t_columns) else "cuda")
    ptrs = (C.c_void_p * max(1, len(t_columns)))(*[t.data_ptr() for t in t_columns])
    args = [ops.ctypes.data_as(C.POINTER(L.StarkAirOp)) if ops.shape[0] else None, ops.shape[0], L.host_ptr(cs), cs.shape[0], ptrs,
            lens.ctypes.data_as(C.POINTER(C.c_uint32)) if lens is not None else None, len(t_columns), int(log2_trace), int(log2_blowup)]
    if spec.offset_arg is not None:
        args.append(L.host_ptr(spec.offset_arg(offset)))
    if spec.rooted:
        args.append(int(root))
    args += [_boundary_table(spec, boundary), len(boundary), _transition_table(spec, transitions), len(transitions), L.device_ptr(t_out), int(out_stride),
             L.stream_ptr(stream)]
    check(getattr(L.lib(), spec.constraints)(*args))
    return t_out


def composition_parts(spec, t_evals, log2_lde, n_parts, evals_stride, offset, root, lde, lens, stream):
    import torch
    from . import _lib as L
    from .errors import check
    P, n_lde = int(n_parts), 1 << int(log2_lde)
    planes = max(P, 1) * spec.width
    t_coeffs = torch.empty(planes * part_block_len(log2_lde, max(P, 1)), dtype=t_evals.dtype, device=t_evals.device)
    t_lde = torch.empty(planes * n_lde, dtype=t_evals.dtype, device=t_evals.device) if lde else None
    ln = (C.c_size_t * max(1, P))()
    args = [L.device_ptr(t_evals), int(evals_stride), int(log2_lde), L.host_ptr(spec.offset_arg(offset))]
    if spec.rooted:
        args.append(int(root))
    args += [P, L.device_ptr(t_coeffs), L.device_ptr(t_lde) if lde else None, ln if lens else None, L.stream_ptr(stream)]
    check(getattr(L.lib(), spec.parts)(*args))
    return t_coeffs, ([int(x) for x in ln] if lens else None), t_lde


# ---- RAP: the auxiliary column of round 1 and the round 2 that reads it (lw_*_aux_fractions_device,
# lw_*_rap_constraint_evaluations_device)
class RapSpec:
    """What a module adds to its Round2Spec for the RAP calls: the ctypes entry of the boundary table whose values are in E,
    the names of the two C calls, and the module's own transform and commitment as callables:
    interpolate(t_in, t_out, log2n, batch, root, stream), lde(t_coeffs, log2_coeffs, t_out, log2n, batch, offset, root, stream),
    commit(t_lde, n_cols, log2n, stream) -> (t_nodes, root)."""

    def __init__(self, r2, boundary, constraints, aux, interpolate, lde, commit):
        self.r2, self.boundary, self.constraints, self.aux = r2, boundary, constraints, aux
        self.interpolate, self.lde, self.commit = interpolate, lde, commit


def _aux_list(spec, side):
    """(constant, [(col, coeff), ...]) -> the constant, the columns and the coefficients as the C call takes them"""
    constant, terms = side
    terms = list(terms)
    cols = np.ascontiguousarray([int(col) for col, _ in terms], dtype=np.uint32)
    return spec.scalars([constant], 1), cols, spec.scalars([coeff for _, coeff in terms], len(terms))


def aux_fractions(rap, t_columns, n, num, den, mode, exclusive, t_out, out_stride, total, count_zeros, stream):
    import torch
    from . import _lib as L
    from .errors import FieldError, check
    spec = rap.r2
    n, stride = int(n), int(out_stride)
    device = t_columns[0].device if len(t_columns) else "cuda"
    if t_out is None:
        t_out = torch.empty(spec.width * max(n, 1), dtype=getattr(torch, spec.torch_word), device=device)
    t_total = torch.empty(max(spec.width, 16 // np.dtype(spec.word).itemsize), dtype=getattr(torch, spec.torch_word), device=device) if total else None
    ptrs = (C.c_void_p * max(1, len(t_columns)))(*[t.data_ptr() for t in t_columns])
    a0, a_cols, a_coeffs = _aux_list(spec, num)
    b0, b_cols, b_coeffs = _aux_list(spec, den)
    u32p = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint32)) if a.shape[0] else None
    zeros = C.c_uint64(0)
    rc = getattr(L.lib(), rap.aux)(ptrs, len(t_columns), n, L.host_ptr(a0), u32p(a_cols), L.host_ptr(a_coeffs) if a_cols.shape[0] else None, a_cols.shape[0],
                                   L.host_ptr(b0), u32p(b_cols), L.host_ptr(b_coeffs) if b_cols.shape[0] else None, b_cols.shape[0],
                                   int(mode) | (L.EXT_AUX_EXCLUSIVE if exclusive else 0), L.device_ptr(t_out), stride,
                                   L.device_ptr(t_total) if total else None, C.byref(zeros) if count_zeros else None, L.stream_ptr(stream))
    try:
        check(rc)
    except FieldError as e:   # LW_ERR_INV_ZERO: the count the call wrote goes with the exception
        e.zero_denominators = int(zeros.value)
        raise
    return t_out, t_total


def _rap_boundary_table(rap, boundary):
    """[(col, step, value, coeff) or (col, step, value, coeff, is_aux)] -> the module's RAP boundary array; value a word of F
    or a scalar of E, coeff a scalar of E"""
    spec = rap.r2
    tab = (rap.boundary * max(1, len(boundary)))()
    for k, entry in enumerate(boundary):
        col, step, value, coeff = entry[:4]
        tab[k].col, tab[k].step, tab[k].is_aux = int(col), int(step), 1 if len(entry) > 4 and entry[4] else 0
        value = tuple(value) if isinstance(value, (tuple, list, np.ndarray)) else (value,) + (0,) * (spec.width - 1)
        tab[k].value[:] = [int(x) for x in spec.scalars([value], 1)[0]]
        tab[k].coeff[:] = [int(x) for x in spec.scalars([coeff], 1)[0]]
    return tab


def rap_constraint_evaluations(rap, program, consts, xconsts, t_columns, t_aux_columns, log2_trace, log2_blowup, boundary, transitions, t_out, out_stride,
                               aux_stride, offset, root, col_log2_len, stream):
    from . import _lib as L
    from .errors import LengthMismatch, check
    from .stark import AIR_OP_DTYPE
    spec = rap.r2
    n_lde = 1 << (int(log2_trace) + int(log2_blowup))
    ops = np.ascontiguousarray(program.ops, dtype=AIR_OP_DTYPE)
    consts = list(consts) if consts is not None else []
    xconsts = list(xconsts) if xconsts is not None else []
    cs = spec.scalars([(c,) * spec.width for c in consts], len(consts))[:, 0].copy()
    xs = spec.scalars(xconsts, len(xconsts))
    if cs.shape[0] < program.n_consts:
        raise LengthMismatch(f"{cs.shape[0]} constants for a program that reads constant {program.n_consts - 1}")
    if xs.shape[0] < program.n_xconsts:
        raise LengthMismatch(f"{xs.shape[0]} extension constants for a program that reads constant {program.n_xconsts - 1}")
    if len(t_columns) < program.n_cols:
        raise LengthMismatch(f"{len(t_columns)} columns for a program that reads column {program.n_cols - 1}")
    if len(t_aux_columns) < program.n_xcols:
        raise LengthMismatch(f"{len(t_aux_columns)} auxiliary columns for a program that reads column {program.n_xcols - 1}")
    lens = None
    if col_log2_len is not None:
        lens = np.ascontiguousarray([int(x) for x in col_log2_len], dtype=np.uint32)
        if lens.shape[0] != len(t_columns):
            raise LengthMismatch(f"{lens.shape[0]} column lengths for {len(t_columns)} columns")
    if t_out is None:
        import torch
        some = t_columns[0] if len(t_columns) else t_aux_columns[0] if len(t_aux_columns) else None
        t_out = torch.empty(spec.width * n_lde, dtype=getattr(torch, spec.torch_word), device=some.device if some is not None else "cuda")
    ptrs = (C.c_void_p * max(1, len(t_columns)))(*[t.data_ptr() for t in t_columns])
    aux_ptrs = (C.c_void_p * max(1, len(t_aux_columns)))(*[t.data_ptr() for t in t_aux_columns])
    args = [ops.ctypes.data_as(C.POINTER(L.StarkAirOp)) if ops.shape[0] else None, ops.shape[0], L.host_ptr(cs), cs.shape[0], L.host_ptr(xs), xs.shape[0], ptrs,
            lens.ctypes.data_as(C.POINTER(C.c_uint32)) if lens is not None else None, len(t_columns), aux_ptrs, len(t_aux_columns), int(aux_stride),
            int(log2_trace), int(log2_blowup), L.host_ptr(spec.offset_arg(offset))]
    if spec.rooted:
        args.append(int(root))
    args += [_rap_boundary_table(rap, boundary), len(boundary), _transition_table(spec, transitions), len(transitions), L.device_ptr(t_out), int(out_stride),
             L.stream_ptr(stream)]
    check(getattr(L.lib(), rap.constraints)(*args))
    return t_out


def round1_aux(rap, t_columns, log2_trace, log2_blowup, num, den, mode, exclusive, offset, root, count_zeros, stream):
    """The second half of round 1: the auxiliary column over the 2^log2_trace rows of the trace columns, the coefficients of
    its planes, their LDE (the module's own, batch = D) and the column commitment over the D planes.
    With count_zeros the column is waited for and a zero denominator raises errors.FieldError (zero_denominators: how many)
    before anything is transformed.  -> (t_aux, t_total, t_polys, t_lde, t_nodes, root)"""
    import torch
    spec = rap.r2
    n, log2_lde = 1 << int(log2_trace), int(log2_trace) + int(log2_blowup)
    t_aux, t_total = aux_fractions(rap, t_columns, n, num, den, mode, exclusive, None, 0, True, count_zeros, stream)
    t_polys = torch.empty_like(t_aux)
    rap.interpolate(t_aux, t_polys, int(log2_trace), spec.width, root, stream)
    t_lde = torch.empty(spec.width << log2_lde, dtype=t_aux.dtype, device=t_aux.device)
    rap.lde(t_polys, int(log2_trace), t_lde, log2_lde, spec.width, offset, root, stream)
    t_nodes, commit_root = rap.commit(t_lde, spec.width, log2_lde, stream)
    return t_aux, t_total, t_polys, t_lde, t_nodes, commit_root
