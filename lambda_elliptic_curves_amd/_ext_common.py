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
