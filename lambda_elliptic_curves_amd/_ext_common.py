"""What the extension-field modules (goldilocks_ext, babybear_ext) share on the host: the shape of their scalars, the
length of a folded block and the loop of the FRI commit phase."""
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
