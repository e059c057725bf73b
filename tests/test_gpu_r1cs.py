"""The resident R1CS on the device (lw_r1cs_*, lw_groth16_h_from_witness*) against tests/r1cs_ref.py, bit for bit in the
stored (Montgomery) form, on Stark252 and BLS12-381 Fr.

The kernels' schedule (lambda_elliptic_curves_amd/csrc/r1cs.hip) and the sizes that cross its boundaries:
  lists    one work-item per output index walks the lists of A, B and C there, 256 outputs per block: 255 | 257 rows.
  split    a list of more than r1cs.SPLIT entries is cut into pieces of SPLIT entries, one work-item each (loads five
           entries at a time); the partials of an output are added by one work-item up to 8 pieces per matrix and by a block
           above, four loads at a time past 4 x 256 pieces: SPLIT | SPLIT + 1 | 2 SPLIT + 1 entries, 8 SPLIT | 8 SPLIT + 1,
           column 0 in each of 3000 rows (100 pieces) and of 33 000 rows (1100 pieces).  The same lists serve bind_rows
           through the transposed index.
  sums     Stark252 carries r1cs.TERMS terms of at most 2p between two reductions: TERMS entries of p - 1 against
           z = p - 1 is the largest such sum.  Fr381 reduces two general terms together.
Both constants are read from the module.  The checks of the compute calls that need a live handle are here as well: they
are decided before any device work, so the made-up addresses they are given are never touched."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import multilinear_ref as M
from tests import r1cs_ref as R
from tests import util
from tests.util import dev, fld

pytestmark = pytest.mark.gpu
FIELDS = ["stark252", "fr381"]
F_REF = {name: M.Fld(M.MODULI[name], True) for name in FIELDS}
BLOCK = 256   # outputs per block of r1cs_lists_kernel, work-items of a block of r1cs_long_kernel
FEW = 8       # R1CS_FEW: an output with at most this many pieces per matrix is added up by one work-item, not by a block


def consts():
    from lambda_elliptic_curves_amd import r1cs
    return r1cs.SPLIT, r1cs.TERMS


def host(t):
    """util.host after the whole device has finished, whichever stream the call used"""
    import torch
    torch.cuda.synchronize()
    return util.host(t)


def ones_dev(n):
    import torch
    return torch.ones((n, 4), dtype=torch.int64, device="cuda")


def pow2(n):
    return 1 << max(0, (n - 1).bit_length())


def rnd_ints(F, n, seed):
    rng = np.random.default_rng(seed)
    return [int.from_bytes(rng.bytes(40), "big") % F.p for _ in range(n)]


def handle(name, n_rows, n_cols, mats):
    from lambda_elliptic_curves_amd import r1cs
    return r1cs.R1cs(fld(name), n_rows, n_cols, [R.csr_arrays(m) for m in mats])


def check_system(name, n_rows, n_cols, mats, seed, z=None, e=None):
    """every product of the system against the restatement: matvec and bind_rows, host and device forms, n_out at its
    least and at the next power of two with the device outputs prefilled with ones, and each device call a second time"""
    F = F_REF[name]
    h = handle(name, n_rows, n_cols, mats)
    z = rnd_ints(F, n_cols, seed) if z is None else z
    e = rnd_ints(F, n_rows, seed + 1) if e is None else e
    c3 = rnd_ints(F, 3, seed + 2)
    want = [R.matvec(F, m, z) for m in mats]
    want_b = R.bind_rows(F, mats, e, c3, n_cols)
    t_z, t_e = dev(R.to_arr(z)), dev(R.to_arr(e))
    for n_out in sorted({n_rows, pow2(n_rows)}):
        exp = [R.to_arr(w + [0] * (n_out - n_rows)) for w in want]
        got = h.matvec(R.to_arr(z), n_out)
        for m in range(3):
            assert got[m].tobytes() == exp[m].tobytes(), ("matvec host", m, n_out)
        outs = [ones_dev(n_out) for _ in range(3)]
        for again in range(2):
            h.matvec_device(t_z, n_out, outs)
            for m in range(3):
                assert host(outs[m]).tobytes() == exp[m].tobytes(), ("matvec device", m, n_out, again)
    # one product at a time leaves the other buffers alone
    only = h.matvec(R.to_arr(z), n_rows, which=(False, True, False))
    assert only[0] is None and only[2] is None and only[1].tobytes() == R.to_arr(want[1]).tobytes()
    for n_out in sorted({n_cols, pow2(n_cols)}):
        exp = R.to_arr(want_b + [0] * (n_out - n_cols))
        assert h.bind_rows(R.to_arr(e), R.to_arr(c3), n_out).tobytes() == exp.tobytes(), ("bind host", n_out)
        out = ones_dev(n_out)
        for again in range(2):
            h.bind_rows_device(t_e, R.to_arr(c3), n_out, out)
            assert host(out).tobytes() == exp.tobytes(), ("bind device", n_out, again)
    return h


def random_mats(F, n_rows, n_cols, per_row, seed, empty=()):
    """three matrices of about per_row entries a row, a third of them one or minus one, columns in no order"""
    rng = np.random.default_rng(seed)
    mats = []
    for m in range(3):
        entries = []
        if m not in empty:
            for i in range(n_rows):
                for _ in range(int(rng.integers(0, 2 * per_row + 1))):
                    kind = int(rng.integers(0, 3))
                    v = F.one if kind == 0 else (F.p - F.one) if kind == 1 else int.from_bytes(rng.bytes(40), "big") % F.p
                    entries.append((i, int(rng.integers(0, n_cols)), v))
        mats.append(R.csr(n_rows, entries))
    return mats


# ---- shapes
@pytest.mark.parametrize("name", FIELDS)
def test_one_by_one(name):
    F = F_REF[name]
    check_system(name, 1, 1, [R.csr(1, [(0, 0, F.elem(3))]), R.csr(1, [(0, 0, F.one)]), R.csr(1, [])], 11)


@pytest.mark.parametrize("name", FIELDS)
@pytest.mark.parametrize("empty", [0, 1, 2])
def test_an_empty_matrix(name, empty):
    check_system(name, 20, 13, random_mats(F_REF[name], 20, 13, 2, 20 + empty, empty=(empty,)), 30 + empty)


@pytest.mark.parametrize("name", FIELDS)
def test_empty_rows_at_the_start_in_the_middle_and_at_the_end(name):
    F = F_REF[name]
    rng = np.random.default_rng(40)
    n_rows, n_cols = 24, 9
    mats = []
    for m in range(3):
        entries = [(i, int(rng.integers(0, n_cols)), int.from_bytes(rng.bytes(40), "big") % F.p)
                   for i in range(n_rows) if i not in (0, 1, 11, 12, 22, 23) for _ in range(2)]
        mats.append(R.csr(n_rows, entries))
    check_system(name, n_rows, n_cols, mats, 41)


@pytest.mark.parametrize("name", FIELDS)
@pytest.mark.parametrize("n_rows", [BLOCK - 1, BLOCK + 1])
def test_rows_around_a_blocks_share(name, n_rows):
    check_system(name, n_rows, 2 * BLOCK + 1, random_mats(F_REF[name], n_rows, 2 * BLOCK + 1, 1, 50 + n_rows), 60)


# ---- split lists
def single_entry_rows(F, n_rows, n_cols, seed, skip=()):
    rng = np.random.default_rng(seed)
    return [(i, int(rng.integers(0, n_cols)), int.from_bytes(rng.bytes(40), "big") % F.p) for i in range(n_rows) if i not in skip]


@pytest.mark.parametrize("name", FIELDS)
@pytest.mark.parametrize("length", ["SPLIT", "SPLIT + 1", "2 SPLIT + 1"])
def test_one_long_row(name, length):
    SPLIT, _ = consts()
    L = {"SPLIT": SPLIT, "SPLIT + 1": SPLIT + 1, "2 SPLIT + 1": 2 * SPLIT + 1}[length]
    F = F_REF[name]
    n_rows, n_cols = 40, 2 * SPLIT + 5
    rng = np.random.default_rng(L)
    mats = []
    for m, row in enumerate((3, 3, 17)):   # A and B share the long row's index, C has its own
        cols = rng.permutation(n_cols)[:L]
        vals = rnd_ints(F, L, 70 + m)
        vals[1], vals[2] = F.one, F.p - F.one
        long_row = [(row, int(j), v) for j, v in zip(cols, vals)]
        mats.append(R.csr(n_rows, single_entry_rows(F, n_rows, n_cols, 80 + m, skip=(row,)) + long_row))
    check_system(name, n_rows, n_cols, mats, 90 + L)


@pytest.mark.parametrize("name", FIELDS)
@pytest.mark.parametrize("length", ["SPLIT", "SPLIT + 1", "2 SPLIT + 1"])
def test_one_long_column(name, length):
    SPLIT, _ = consts()
    L = {"SPLIT": SPLIT, "SPLIT + 1": SPLIT + 1, "2 SPLIT + 1": 2 * SPLIT + 1}[length]
    F = F_REF[name]
    n_rows, n_cols = 2 * SPLIT + 5, 40
    rng = np.random.default_rng(L + 1)
    mats = []
    for m, col in enumerate((3, 3, 17)):
        rows = rng.permutation(n_rows)[:L]
        vals = rnd_ints(F, L, 100 + m)
        vals[0], vals[3] = F.p - F.one, F.one
        # the other rows avoid the long column, so that its length is exact
        others = [(i, j if j != col else j + 1, v) for i, j, v in single_entry_rows(F, n_rows, n_cols - 1, 110 + m)]
        mats.append(R.csr(n_rows, others + [(int(i), col, v) for i, v in zip(rows, vals)]))
    check_system(name, n_rows, n_cols, mats, 120 + L)


@pytest.mark.parametrize("name", FIELDS)
def test_the_constant_column_in_every_row(name):
    F = F_REF[name]
    n_rows, n_cols = 3000, 50
    rng = np.random.default_rng(130)
    gen = lambda: int.from_bytes(rng.bytes(40), "big") % F.p
    a = [(i, 0, F.one) for i in range(n_rows)] + [(i, int(rng.integers(1, n_cols)), gen()) for i in range(n_rows)]
    b = [(i, 0, gen()) for i in range(n_rows)]
    c = [(i, int(rng.integers(0, n_cols)), F.p - F.one) for i in range(n_rows)]
    h = check_system(name, n_rows, n_cols, [R.csr(n_rows, a), R.csr(n_rows, b), R.csr(n_rows, c)], 131)
    assert h.n_rows == n_rows


@pytest.mark.parametrize("name", FIELDS)
def test_lists_around_the_two_ways_of_adding_partials(name):
    """FEW pieces are added by one work-item, FEW + 1 by a block: rows of FEW SPLIT and FEW SPLIT + 1 entries side by side"""
    SPLIT, _ = consts()
    F = F_REF[name]
    n_rows, n_cols = 6, FEW * SPLIT + 2
    rng = np.random.default_rng(125)
    mats = []
    for m, (row_few, row_many) in enumerate(((1, 2), (2, 1), (4, 5))):
        ent = []
        for row, L in ((row_few, FEW * SPLIT), (row_many, FEW * SPLIT + 1)):
            ent += [(row, int(j), v) for j, v in zip(rng.permutation(n_cols)[:L], rnd_ints(F, L, 126 + m + row))]
        mats.append(R.csr(n_rows, ent + [(0, 3, F.one)]))
    check_system(name, n_rows, n_cols, mats, 127)


@pytest.mark.parametrize("name", FIELDS)
def test_a_column_of_more_partials_than_four_a_work_item(name):
    """a block adds its partials four loads at a time once there are more than 4 x 256 of them: column 0 in 33 000 rows is
    1100 pieces, the unrolled loop for some work-items and the plain one for the rest.  Only this size reaches that loop."""
    SPLIT, _ = consts()
    F = F_REF[name]
    n_rows, n_cols = 33000, 7
    assert n_rows > 4 * BLOCK * SPLIT
    rng = np.random.default_rng(128)
    vals = rnd_ints(F, 64, 129)
    a = R.csr(n_rows, [(i, 0, vals[i % 64] if i % 3 else F.one) for i in range(n_rows)])
    b = R.csr(n_rows, [(i, int(rng.integers(1, n_cols)), F.p - F.one) for i in range(0, n_rows, 7)])
    h = handle(name, n_rows, n_cols, [a, b, R.csr(n_rows, [])])
    e, c3 = rnd_ints(F, n_rows, 130), rnd_ints(F, 3, 131)
    want = R.to_arr(R.bind_rows(F, [a, b, R.csr(n_rows, [])], e, c3, n_cols))
    for again in range(2):
        assert h.bind_rows(R.to_arr(e), R.to_arr(c3)).tobytes() == want.tobytes()


# ---- arithmetic edges
@functools.lru_cache(maxsize=None)
def edge_system(name):
    SPLIT, TERMS = consts()
    F = F_REF[name]
    top, neg = F.p - 1, F.p - F.one
    n_cols = SPLIT + TERMS + 3
    rows = [
        [(j, top) for j in range(TERMS)],                               # 0: one full group of the largest general terms
        [(j, neg) for j in range(TERMS)],                               # 1: the class minus one
        [(j, F.one) for j in range(TERMS)],                             # 2: the class one
        [(j, top) for j in range(2 * TERMS)],                           # 3: two full groups
        [(j, top) for j in range(TERMS + 1)],                           # 4: a full group and one term
        [(0, 0), (1, top), (2, 0), (3, F.one), (4, 0)],                 # 5: explicit zeros
        [(2, top), (2, top), (2, neg), (5, F.one), (2, F.elem(7))],     # 6: a repeated (row, column)
        [(9, top), (1, neg), (7, F.one), (0, top), (4, F.elem(2))],     # 7: columns in no order
        [(j, neg) for j in range(SPLIT + TERMS)],                       # 8: pieces of minus ones
        [(j, top) for j in range(SPLIT + TERMS + 3)],                   # 9: pieces of the largest general terms
        [],                                                             # 10
    ]
    mat = R.csr(len(rows), [(i, j, v) for i, r in enumerate(rows) for j, v in r])
    rot = lambda k: R.csr(len(rows), [((i + k) % len(rows), j, v) for i, r in enumerate(rows) for j, v in r])
    return len(rows), n_cols, (mat, rot(3), rot(7))


@pytest.mark.parametrize("name", FIELDS)
@pytest.mark.parametrize("vector", ["p - 1", "zero", "one", "random"])
def test_sums_at_their_bound(name, vector):
    F = F_REF[name]
    n_rows, n_cols, mats = edge_system(name)
    fill = {"p - 1": F.p - 1, "zero": 0, "one": F.one}.get(vector)
    z = rnd_ints(F, n_cols, 140) if fill is None else [fill] * n_cols
    e = rnd_ints(F, n_rows, 141) if fill is None else [fill] * n_rows
    check_system(name, n_rows, n_cols, list(mats), 142, z=z, e=e)


# ---- whole calls
@functools.lru_cache(maxsize=None)
def skewed_case(name):
    """600 x 300 with a long row, a heavy column and the classes mixed; its handle and restated matrices"""
    F = F_REF[name]
    mats = random_mats(F, 600, 300, 1, 150)
    rng = np.random.default_rng(151)
    extra = [(i, 0, F.one) for i in range(0, 600, 2)] + [(77, int(j), int.from_bytes(rng.bytes(40), "big") % F.p) for j in rng.permutation(300)[:70]]
    rp, ci, va = mats[0]
    a = R.csr(600, [(i, ci[k], va[k]) for i in range(600) for k in range(rp[i], rp[i + 1])] + extra)
    mats = [a, mats[1], mats[2]]
    return mats, handle(name, 600, 300, mats)


@pytest.mark.parametrize("name", FIELDS)
def test_bind_rows_with_unit_coefficients_is_the_transposed_product(name):
    F = F_REF[name]
    mats, h = skewed_case(name)
    e = rnd_ints(F, 600, 152)
    for m in range(3):
        rp, ci, va = mats[m]
        transposed = R.csr(300, [(ci[k], i, va[k]) for i in range(600) for k in range(rp[i], rp[i + 1])])
        c3 = [F.one if k == m else 0 for k in range(3)]
        assert h.bind_rows(R.to_arr(e), R.to_arr(c3)).tobytes() == R.to_arr(R.matvec(F, transposed, e)).tobytes()


@pytest.mark.parametrize("name", FIELDS)
def test_inner_product_identity(name):
    """<e, cA Az + cB Bz + cC Cz> = <bind_rows(e), z> from the device's own outputs"""
    F = F_REF[name]
    mats, h = skewed_case(name)
    e, z, c3 = rnd_ints(F, 600, 160), rnd_ints(F, 300, 161), rnd_ints(F, 3, 162)
    prods = [R.to_ints(x) for x in h.matvec(R.to_arr(z))]
    bound = R.to_ints(h.bind_rows(R.to_arr(e), R.to_arr(c3)))
    lhs = sum(F.mul(e[i], sum(F.mul(c, pr[i]) for c, pr in zip(c3, prods)) % F.p) for i in range(600)) % F.p
    assert lhs == sum(F.mul(b, zj) for b, zj in zip(bound, z)) % F.p


def satisfied_system(F, n_rows, seed):
    """row i: z[a_i] * z[b_i] = z[k + i] over earlier variables, a fresh variable per row; -> (mats, n_cols, z)"""
    rng = np.random.default_rng(seed)
    k = 8
    z = [F.one] + rnd_ints(F, k - 1, seed + 1)
    ent = [[], [], []]
    for i in range(n_rows):
        a, b = int(rng.integers(0, k + i)), int(rng.integers(0, k + i))
        ent[0].append((i, a, F.one))
        ent[1].append((i, b, F.one))
        ent[2].append((i, k + i, F.one))
        z.append(F.mul(z[a], z[b]))
    return [R.csr(n_rows, x) for x in ent], k + n_rows, z


@pytest.mark.parametrize("name", FIELDS)
def test_first_unsatisfied_takes_the_minimum_over_blocks(name):
    F = F_REF[name]
    n_rows = 1500
    mats, n_cols, z = satisfied_system(F, n_rows, 170)
    h = handle(name, n_rows, n_cols, mats)
    assert R.first_unsatisfied(F, mats, z) == -1
    assert h.first_unsatisfied(R.to_arr(z)) == -1 and h.first_unsatisfied_device(dev(R.to_arr(z))) == -1
    bad = list(z)
    for row in (1200, 300):   # the fresh variables of two rows five blocks apart
        bad[8 + row] = (bad[8 + row] + 1) % F.p
    az, bz, cz = (R.matvec(F, m, bad) for m in mats)
    broken = [i for i in range(n_rows) if F.mul(az[i], bz[i]) != cz[i]]
    assert broken[0] == 300 and 1200 in broken and len({i // BLOCK for i in broken}) >= 2
    assert R.first_unsatisfied(F, mats, bad) == 300
    for again in range(2):
        assert h.first_unsatisfied(R.to_arr(bad)) == 300
        assert h.first_unsatisfied_device(dev(R.to_arr(bad))) == 300
    only_late = list(z)
    only_late[8 + n_rows - 1] = (only_late[8 + n_rows - 1] + 1) % F.p
    assert h.first_unsatisfied(R.to_arr(only_late)) == n_rows - 1


@functools.lru_cache(maxsize=None)
def circom_case(fixture):
    from lambda_elliptic_curves_amd import r1cs
    F = F_REF["fr381"]
    r1, w = R.fixture(fixture)
    return R.circom_mats(F, r1), w, r1cs.R1cs.from_circom(r1)


@pytest.mark.parametrize("fixture", ["vitalik", "poseidon"])
def test_circom_fixture(fixture):
    F = F_REF["fr381"]
    mats, w, h = circom_case(fixture)
    assert h.first_unsatisfied(R.to_arr(w)) == -1 and h.first_unsatisfied_device(dev(R.to_arr(w))) == -1
    got = h.matvec(R.to_arr(w), pow2(h.n_rows))
    for m in range(3):
        assert got[m].tobytes() == R.to_arr(R.matvec(F, mats[m], w, pow2(h.n_rows))).tobytes()
    bad = list(w)
    bad[h.n_cols // 2] = (bad[h.n_cols // 2] + 1) % F.p
    want = R.first_unsatisfied(F, mats, bad)
    assert want >= 0 and h.first_unsatisfied(R.to_arr(bad)) == want


def test_from_dense_drops_zeros_and_matches():
    from lambda_elliptic_curves_amd import r1cs
    F = F_REF["stark252"]
    a, b, c = [[1, 0, F.p - 1], [0, 0, 0]], [[0, 2, 0], [5, 0, 0]], [[0, 0, 0], [0, 0, 9]]
    h = r1cs.R1cs.from_dense(fld("stark252"), a, b, c)
    z = rnd_ints(F, 3, 180)
    mats = [R.csr(2, [(i, j, F.elem(v)) for i, row in enumerate(d) for j, v in enumerate(row) if v]) for d in (a, b, c)]
    got = h.matvec(R.to_arr(z))
    for m in range(3):
        assert got[m].tobytes() == R.to_arr(R.matvec(F, mats[m], z)).tobytes()


# ---- the checks that need a live handle: decided before any device work, the addresses are made up
@pytest.mark.parametrize("name", FIELDS)
def test_live_handle_argument_checks(name):
    from lambda_elliptic_curves_amd import _lib as L
    F = F_REF[name]
    h = handle(name, 4, 6, [R.csr(4, [(0, 0, F.one)])] * 3)
    lib = C.CDLL(L.LIB_PATH)
    vp, sz, N = C.c_void_p, C.c_size_t, C.c_void_p(None)
    H = h._h
    base = 0x7f0000000000   # 6 columns = 192 bytes of z, 4 rows = 128 bytes of e
    Z, A, B, Cz = vp(base), vp(base + 0x1000), vp(base + 0x2000), vp(base + 0x3000)
    row = C.c_int64(7)
    coeffs = R.to_arr([F.one, F.one, F.one])
    c3 = vp(coeffs.ctypes.data)
    cases = [
        ("matvec n_out below the rows", lambda: lib.lw_r1cs_matvec_device(H, Z, sz(3), A, B, Cz, N)),
        ("matvec null z", lambda: lib.lw_r1cs_matvec_device(H, N, sz(4), A, B, Cz, N)),
        ("matvec misaligned z", lambda: lib.lw_r1cs_matvec_device(H, vp(base + 8), sz(4), A, B, Cz, N)),
        ("matvec misaligned output", lambda: lib.lw_r1cs_matvec_device(H, Z, sz(4), A, vp(base + 0x2008), Cz, N)),
        ("matvec output overlaps z", lambda: lib.lw_r1cs_matvec_device(H, Z, sz(4), vp(base + 176), B, Cz, N)),
        ("matvec output ends in z", lambda: lib.lw_r1cs_matvec_device(H, vp(base + 0x1000 + 112), sz(4), A, B, Cz, N)),
        ("matvec outputs overlap", lambda: lib.lw_r1cs_matvec_device(H, Z, sz(4), A, vp(base + 0x1000 + 96), Cz, N)),
        ("matvec same output twice", lambda: lib.lw_r1cs_matvec_device(H, Z, sz(4), A, N, A, N)),
        ("matvec padding overlaps", lambda: lib.lw_r1cs_matvec_device(H, Z, sz(0x1000 // 32 + 1), A, B, N, N)),
        ("matvec host outputs overlap", lambda: lib.lw_r1cs_matvec(H, Z, sz(4), A, A, N)),
        ("bind n_out below the columns", lambda: lib.lw_r1cs_bind_rows_device(H, Z, c3, sz(5), A, N)),
        ("bind null coefficients", lambda: lib.lw_r1cs_bind_rows_device(H, Z, N, sz(6), A, N)),
        ("bind null output", lambda: lib.lw_r1cs_bind_rows_device(H, Z, c3, sz(6), N, N)),
        ("bind misaligned e", lambda: lib.lw_r1cs_bind_rows_device(H, vp(base + 4), c3, sz(6), A, N)),
        ("bind misaligned output", lambda: lib.lw_r1cs_bind_rows_device(H, Z, c3, sz(6), vp(base + 0x1010 - 8), N)),
        ("bind output overlaps e", lambda: lib.lw_r1cs_bind_rows_device(H, Z, c3, sz(6), vp(base + 96), N)),
        ("bind host output overlaps e", lambda: lib.lw_r1cs_bind_rows(H, Z, c3, sz(6), vp(base + 96))),
        ("check null z", lambda: lib.lw_r1cs_first_unsatisfied_device(H, N, C.byref(row), N)),
        ("check null out", lambda: lib.lw_r1cs_first_unsatisfied_device(H, Z, N, N)),
        ("check misaligned z", lambda: lib.lw_r1cs_first_unsatisfied_device(H, vp(base + 8), C.byref(row), N)),
    ]
    assert {k: f() for k, f in cases} == {k: L.ERR_BAD_ARG for k, _ in cases}
    assert row.value == 7


# ---- Groth16 h from the witness
def check_h(h, w_ints, gates, satisfied):
    from lambda_elliptic_curves_amd import fft, groth16
    from tests import util
    w = R.to_arr(w_ints)
    got = groth16.h_from_witness(h, w, gates)
    lro = [fft.interpolate_fft(fft.FrField, x) for x in h.matvec(w, gates)]
    assert got.tobytes() == groth16.calculate_h_coefficients(*lro, gates).tobytes()
    exp = util.groth16_h_by_composition(*lro, gates)
    assert got.shape == exp.shape and got.tobytes() == np.ascontiguousarray(exp).tobytes()
    full = groth16.h_from_witness(h, w, gates, strip=False)
    t_h, n = groth16.h_from_witness_device(h, dev(w), gates, want_len=True)
    assert n == got.shape[0] and host(t_h).tobytes() == full.tobytes()
    assert host(groth16.h_from_witness_device(h, dev(w), gates)).tobytes() == full.tobytes()   # a second call, no length
    if satisfied:
        assert got.shape[0] <= gates - 1


@pytest.mark.parametrize("fixture", ["vitalik", "poseidon"])
def test_h_from_witness_on_the_circom_fixtures(fixture):
    _, w, h = circom_case(fixture)
    check_h(h, w, pow2(h.n_rows), True)


@pytest.mark.parametrize("n_rows", [1, 3, 64, 213])
def test_h_from_witness_on_random_unsatisfied_systems(n_rows):
    F = F_REF["fr381"]
    n_cols = n_rows + 5
    mats = random_mats(F, n_rows, n_cols, 2, 190 + n_rows)
    h = handle("fr381", n_rows, n_cols, mats)
    check_h(h, rnd_ints(F, n_cols, 191 + n_rows), pow2(n_rows), False)
    if n_rows == 3:
        check_h(h, rnd_ints(F, n_cols, 192), 16, False)   # more gates than the next power of two


def test_h_from_witness_argument_checks():
    from lambda_elliptic_curves_amd import errors, groth16
    F = F_REF["fr381"]
    h = handle("fr381", 3, 4, random_mats(F, 3, 4, 1, 200))
    w = R.to_arr(rnd_ints(F, 4, 201))
    with pytest.raises(errors.InputError):
        groth16.h_from_witness(h, w, 6)
    with pytest.raises(errors.HipError):
        groth16.h_from_witness(h, w, 2)       # fewer gates than constraints
    S = F_REF["stark252"]
    hs = handle("stark252", 3, 4, random_mats(S, 3, 4, 1, 202))
    with pytest.raises(errors.HipError):
        groth16.h_from_witness(hs, R.to_arr(rnd_ints(S, 4, 203)), 4)   # Groth16 runs over Fr381


# ---- Spartan's first round, end to end
@pytest.mark.parametrize("fixture", ["vitalik", "poseidon"])
def test_spartan_first_round_sums_to_zero(fixture):
    from lambda_elliptic_curves_amd import fft, multilinear
    F = F_REF["fr381"]
    _, w, h = circom_case(fixture)
    n = pow2(h.n_rows).bit_length() - 1
    n = max(n, 1)
    t_a, t_b, t_c = h.matvec_device(dev(R.to_arr(w)), 1 << n)
    tau = R.to_arr(rnd_ints(F, n, 210))
    t_eq = multilinear.eq_table_device(fft.FrField, tau)
    minus_one = R.to_arr([F.p - F.one])[0]
    g = multilinear.sumcheck_terms_round_device(fft.FrField, [t_a, t_b, t_c], [(None, (0, 1)), (minus_one, (2,))], n, t_eq)
    g = R.to_ints(g)
    assert len(g) == 4 and (g[0] + g[1]) % F.p == 0
