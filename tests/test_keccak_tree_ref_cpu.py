"""The plain references of tests/keccak_tree_ref.py against the oracle's compiled ones, on the CPU: the tree written from
its definition equals O.merkle_commit_columns[_babybear] at every column count the sponge-seam tests use, and the fold in
Python integers equals O.fri_fold_twice over the edge operands."""
import numpy as np
import pytest

from oracle import bigint_def as D
from oracle import oracle as O
from tests import keccak_tree_ref as K
from tests import util

LAYOUT_OF = {32: "stark252", 8: "babybear_u64", 4: "babybear_u32"}
SEAMS = [(eb, n_cols) for eb in (32, 8, 4) for n_cols in K.SEAM_COLS[eb]] + [(-32, 4), (-32, 17)]   # -32: Fr381 values
FIELDS = {"stark252": (O.F_STARK252, D.P_STARK252), "fr381": (O.F_FR381, D.P_FR381)}


def seam_columns(eb, n_cols, n, seed=4100):
    name = "fr381" if eb < 0 else LAYOUT_OF[eb]
    return np.stack([util.rand_elems(name, n, seed + 5 * c + n_cols) for c in range(n_cols)])


@pytest.mark.parametrize("bit_reverse", [False, True])
@pytest.mark.parametrize("eb,n_cols", SEAMS)
def test_plain_tree_equals_the_oracle(eb, n_cols, bit_reverse):
    cols = seam_columns(eb, n_cols, 4)
    assert K.elem_bytes(cols) == abs(eb)
    exp = O.merkle_commit_columns(cols, bit_reverse) if abs(eb) == 32 else O.merkle_commit_columns_babybear(cols, bit_reverse)
    got = K.keccak_tree(cols, bit_reverse)
    assert got.shape == exp.shape == (7, 32)
    assert got.tobytes() == exp.tobytes()
    if bit_reverse:   # rows 1 and 2 trade places: the permutation is seen
        assert got.tobytes() != K.keccak_tree(cols, False).tobytes()


def test_plain_tree_of_one_row_is_its_leaf():
    cols = seam_columns(32, 1, 1)
    assert K.keccak_tree(cols, True).tobytes() == O.keccak256(cols.astype(">u8").tobytes()) == O.merkle_commit_columns(cols, True).tobytes()


def test_bitrev():
    assert [K.bitrev(i, 3) for i in range(8)] == [0, 4, 2, 6, 1, 5, 3, 7] and K.bitrev(0, 0) == 0
    assert K.bitrev(1, 17) == 1 << 16


@pytest.mark.parametrize("name", ["stark252", "fr381"])
def test_stored_form_is_the_value_times_2_256(name):
    f, p = FIELDS[name]
    e = K.edge_values(p)
    assert util.to_ints(O.elems_to_mont(f, e)) == [v * K.R256 % p for v in e]


@pytest.mark.parametrize("reading", ["stored", "canonical"])
@pytest.mark.parametrize("name", ["stark252", "fr381"])
def test_fold_reference_equals_python_integers_at_the_edges(name, reading):
    """The edge operands both as the stored words themselves (the additions of the stored residues cross p) and as the
    values they stand for (zeta = 0, 1, -1)."""
    f, p = FIELDS[name]
    to_stored = (lambda v: v) if reading == "stored" else (lambda v: v * K.R256 % p)
    coeffs = [to_stored(v) for v in K.edge_coeffs(p)]
    assert len(coeffs) == 99
    zetas = [to_stored(z) for z in K.edge_values(p)] + [util.to_ints(util.rand_elems(name, 1, 77))[0]]
    for z in zetas:
        exp = K.fold_twice_stored(p, coeffs, z)
        got = O.fri_fold_twice(f, util.to_arr(coeffs), util.to_arr([z]), strip=False)
        assert len(exp) == 50 and all(v < p for v in exp)
        assert util.to_ints(got) == exp
    # zeta = 1 in the canonical reading is the plain sum of the pair, doubled
    if reading == "canonical":
        e = K.edge_coeffs(p)
        one = K.fold_twice_stored(p, coeffs, K.R256 % p)
        assert one == [2 * (e[2 * i] + (e[2 * i + 1] if 2 * i + 1 < 99 else 0)) % p * K.R256 % p for i in range(50)]
