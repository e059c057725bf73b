"""The Keccak-256 column commitment and the doubled FRI fold written out from their definitions, on Python bytes and
integers: what the tests of csrc/merkle.hip and csrc/fri.hip compare against at small sizes, and what
tests/test_keccak_tree_ref_cpu.py holds against the oracle's compiled versions.

    leaf_i = keccak256(as_bytes(col_0[r]) || as_bytes(col_1[r]) || ...)     r = bitrev(i) or i
    parent = keccak256(left || right)                                        nodes stored root first
    as_bytes = the element's raw words big-endian: 4 bytes (u32), 8 bytes (one u64 limb) or 4 x 8 bytes (limbs MS first)
"""
import numpy as np

from oracle import oracle as O

R256 = 1 << 256   # the Montgomery radix of the two 256-bit fields

# column counts at log2n = 3 whose leaves put the padding at every seam of the rate (136 bytes = 17 lanes): leaf bytes
# 128 / 256 / 416 / 544 / 672 (32-byte elements), 128 / 136 / 144 / 272 / 400 (8-byte), 124 / 128 / 132 / 136 / 140 / 260 / 268 /
# 272 (4-byte: an odd count leaves half a lane before the 0x01 byte)
SEAM_COLS = {32: (4, 8, 13, 17, 21), 8: (16, 17, 18, 34, 50), 4: (31, 32, 33, 34, 35, 65, 67, 68)}


def bitrev(i, bits):
    return int(format(i, "0%db" % bits)[::-1], 2) if bits else 0


def elem_bytes(columns):
    """bytes of one element of (n_cols, n, 4) uint64, (n_cols, n) uint64 or (n_cols, n) uint32 columns"""
    return 32 if columns.ndim == 3 else columns.dtype.itemsize


def keccak_tree(columns, bit_reverse):
    """-> (2n - 1, 32) uint8 nodes, root first, of the tree over the rows of `columns`"""
    cols = np.ascontiguousarray(columns)
    n_cols, n = cols.shape[0], cols.shape[1]
    log2n = n.bit_length() - 1
    assert 1 << log2n == n
    word = cols.dtype.itemsize
    as_bytes = lambda e: b"".join(int(w).to_bytes(word, "big") for w in np.atleast_1d(e))
    level = []
    for i in range(n):
        r = bitrev(i, log2n) if bit_reverse else i
        level.append(O.keccak256(b"".join(as_bytes(cols[c, r]) for c in range(n_cols))))
    levels = [level]
    while len(level) > 1:
        level = [O.keccak256(level[2 * k] + level[2 * k + 1]) for k in range(len(level) // 2)]
        levels.append(level)
    return np.frombuffer(b"".join(b"".join(lv) for lv in reversed(levels)), np.uint8).reshape(2 * n - 1, 32)


def edge_values(p):
    """operands at which an addition mod p just crosses, or just misses, the modulus"""
    return [0, 1, 2, p - 1, p - 2, (p - 1) // 2, (p + 1) // 2]


def edge_coeffs(p):
    """every ordered pair (c0, c1) of edge values, then one unpaired p - 1"""
    e = edge_values(p)
    return [v for c0 in e for c1 in e for v in (c0, c1)] + [p - 1]


def fold_twice_stored(p, stored, zeta_stored):
    """2 * (c0 + zeta * c1) per pair (an unpaired last c0 alone) on elements in stored (Montgomery, radix 2^256) form,
    as integers: out of the stored form, the arithmetic of the definition, back.  All ceil(n/2) results, nothing stripped."""
    rinv = pow(R256, -1, p)
    c = [v * rinv % p for v in stored]
    z = zeta_stored * rinv % p
    out = []
    for i in range((len(c) + 1) // 2):
        c1 = c[2 * i + 1] if 2 * i + 1 < len(c) else 0
        out.append(2 * (c[2 * i] + z * c1) % p * R256 % p)
    return out
