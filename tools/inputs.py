"""Synthetic inputs for the tools/ scripts, in the reference's memory layout, WITHOUT the CPU checker (tests/util.py pulls in
oracle/, which only tests/, smoke() and bench.py's cpu_baseline leg may use)."""
import numpy as np

P_BABYBEAR = 2013265921
P_STARK252 = 0x800000000000011000000000000000000000000000000000000000000000001
P_FR381 = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001
P_GOLDILOCKS = (1 << 64) - (1 << 32) + 1


def field_pairs():
    """name -> (product Field, None): the shape of tests/util.field_pairs() without the checker's field ids"""
    from lambda_elliptic_curves_amd import fft
    return {"stark252": (fft.Stark252PrimeField, None), "fr381": (fft.FrField, None),
            "babybear_u64": (fft.Babybear31PrimeField, None), "babybear_u32": (fft.Babybear31PrimeFieldU32, None),
            "babybear_ext4": (fft.Degree4BabyBearExtensionField, None)}


def curve_pairs():
    from lambda_elliptic_curves_amd import msm
    return {"bls12_381_g1": (msm.BLS12381Curve, None), "bn254_g1": (msm.BN254Curve, None),
            "bn254_g2": (msm.BN254TwistCurve, None), "bls12_381_g2": (msm.BLS12381TwistCurve, None)}


def rand_elems(name, n, seed):
    """n canonical residues (any value < p is a valid Montgomery-form element)"""
    rng = np.random.default_rng(seed)
    if name in ("stark252", "fr381"):
        a = rng.integers(0, 1 << 63, size=(n, 4), dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, size=(n, 4), dtype=np.uint64)
        a[:, 0] &= np.uint64((1 << (59 if name == "stark252" else 62)) - 1)
        return a
    if name == "babybear_u32":
        return rng.integers(0, P_BABYBEAR, size=n, dtype=np.uint32)
    if name == "babybear_u64":
        return rng.integers(0, P_BABYBEAR, size=n, dtype=np.uint64)
    if name == "babybear_ext4":
        return rng.integers(0, P_BABYBEAR, size=(n, 4), dtype=np.uint64)
    if name == "goldilocks":
        return rng.integers(0, P_GOLDILOCKS, size=n, dtype=np.uint64)
    raise KeyError(name)


def r1cs_system(name, n_rows, n_cols, skewed, seed):
    """A synthetic R1CS for tools/r1cs_timing.py: three CSR matrices (row_ptr, col_idx, values) as arrays.
    skewed: the row and column profile of the circom Poseidon circuit as the timing asks for it - every row one entry, one
    row in 512 a long one of 58 entries (about 1.11 entries a row), and in C the constant column 0 as the entry of 30 % of
    the rows.  Otherwise the same number of entries spread evenly: one a row, the rest as second entries of rows picked
    at random, every column drawn uniformly.  Values: 45 % one, 45 % minus one, 10 % general."""
    p = P_STARK252 if name == "stark252" else P_FR381
    word = lambda v: np.array([(v >> (64 * (3 - k))) & ((1 << 64) - 1) for k in range(4)], dtype=np.uint64)
    one, minus_one = word((1 << 256) % p), word(p - (1 << 256) % p)
    rng = np.random.default_rng(seed)
    mats = []
    for m in range(3):
        long_rows = rng.permutation(n_rows)[:n_rows // 512]
        extra = 57 * long_rows.shape[0]
        lens = np.ones(n_rows, np.int64)
        if skewed:
            lens[long_rows] = 58
        else:
            lens[rng.permutation(n_rows)[:extra]] += 1
        row_ptr = np.zeros(n_rows + 1, np.uint32)
        row_ptr[1:] = np.cumsum(lens)
        nnz = int(row_ptr[-1])
        cols = rng.integers(0, n_cols, nnz, dtype=np.uint32)
        if skewed and m == 2:
            first = row_ptr[:-1][rng.random(n_rows) < 0.3]
            cols[first] = 0
        values = rand_elems(name, nnz, seed + 10 + m)
        kind = rng.random(nnz)
        values[kind < 0.45] = one
        values[(kind >= 0.45) & (kind < 0.9)] = minus_one
        mats.append((row_ptr, cols, values))
    return mats


def offset_elem(name, h):
    """Coset offset h (small canonical int) as one domain-field element in memory (Montgomery) form"""
    if name == "babybear_u32":
        return np.array([h * (1 << 32) % P_BABYBEAR], dtype=np.uint32)
    if name in ("babybear_u64", "babybear_ext4"):
        return np.array([h * (1 << 64) % P_BABYBEAR], dtype=np.uint64)
    p = P_STARK252 if name == "stark252" else P_FR381
    m = h * (1 << 256) % p
    return np.array([(m >> (64 * (3 - k))) & ((1 << 64) - 1) for k in range(4)], dtype=np.uint64)
