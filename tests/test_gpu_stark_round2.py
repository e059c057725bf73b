"""STARK round 2 on the device (csrc/stark_round2.hip) against tests/stark_round2_ref.py, the Python big-integer
restatement of ConstraintEvaluator::evaluate, break_in_parts and commit_composition_polynomial, and against the values
the reference's Stone-compatibility tests assert (tests/golden/stark_round2.json).  Field arithmetic is exact: every
comparison is byte equality in the stored (Montgomery) form."""
import json
import os

import numpy as np
import pytest

from oracle import bigint_def as D
from oracle import oracle as O
from tests import stark_query_ref as Q
from tests import stark_round2_ref as R2
from tests import util

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODULI = {"stark252": D.P_STARK252, "fr381": D.P_FR381}
OIDS = {"stark252": O.F_STARK252, "fr381": O.F_FR381}


def fld(name):
    from lambda_elliptic_curves_amd import fft
    return {"stark252": fft.Stark252PrimeField, "fr381": fft.FrField}[name]


def cuda(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).cuda()


def host(t):
    return t.cpu().numpy().view(np.uint64)


def rand_ints(p, n, seed):
    rng = np.random.default_rng(seed)
    return [int.from_bytes(rng.bytes(32), "big") % p for _ in range(n)]


# ---- batch inversion

def inverse_sizes():
    from lambda_elliptic_curves_amd import poly
    B = poly.batch_inverse_block()
    return B, [1, 2, 63, 64, 65, 255, 256, 257, B - 1, B, B + 1, 3 * B + 5]


@pytest.mark.parametrize("name", ["stark252", "fr381"])
def test_batch_inverse_matches_python_pow(name):
    import torch
    from lambda_elliptic_curves_amd import poly
    p, F = MODULI[name], fld(name)
    _B, sizes = inverse_sizes()
    edge = [1, 2, p - 1, p - 2, pow(1 << 256, -1, p)]          # the last one is stored as 1
    nmax = max(sizes)
    vals = (edge + [v or 1 for v in rand_ints(p, nmax, 77)])[:nmax]
    stored = R2.to_stored(p, vals)
    want = R2.to_stored(p, [pow(v, -1, p) for v in vals])
    assert O.array_to_ints(stored[4:5]) == [1]
    for n in sizes:
        t_in = cuda(stored[:n])
        t_out = torch.zeros_like(t_in)
        poly.batch_inverse_device(F, t_in, n, t_out)                                   # out of place
        got = host(t_out)
        assert all(v < p for v in O.array_to_ints(got)), (name, n)
        assert np.array_equal(got, want[:n]), (name, n)
        assert np.array_equal(host(t_in), stored[:n])
        poly.batch_inverse_device(F, t_in, n)                                          # in place
        assert np.array_equal(host(t_in), want[:n]), (name, n)
    assert np.array_equal(poly.batch_inverse(F, stored[:259]), want[:259])             # host form
    assert poly.batch_inverse(F, np.zeros((0, 4), np.uint64)).shape == (0, 4)


@pytest.mark.parametrize("name", ["stark252", "fr381"])
def test_batch_inverse_of_chosen_stored_values(name):
    """fe_inv_fast on operands of our choosing.  field_batch_inverse_kernel gives work-item t the elements t + 256 j of a
    block and inverts their product, so in the test above an edge value reaches the binary GCD multiplied into random
    neighbours.  With n <= 256 every work-item owns exactly one element and the GCD sees the stored value itself: the
    edge set, 2^k, 2^k +- 1 and p - 2^k for every bit k, and 2000 values with p's top two limbs (the Z families of
    tests/test_gpu_ec_pointwise.py).  One launch of n = B has the chosen value at position t and R mod p (the stored one)
    in the seven other places of its chunk.  Expected: pow(v R^-1, -1, p) R mod p."""
    import torch
    from lambda_elliptic_curves_amd import poly
    from tests import ec_formulas_ref as E
    p, F = MODULI[name], fld(name)
    B, _sizes = inverse_sizes()
    R = 1 << 256
    vals = E.inverse_operands(p, 4, 31)
    assert len(vals) > 2000 + 3 * p.bit_length() and all(0 < v < p for v in vals)
    stored = O.ints_to_array(vals, 4)
    want = O.ints_to_array([pow(v * pow(R, -1, p), -1, p) * R % p for v in vals], 4)
    for at in range(0, len(vals), 256):
        n = min(256, len(vals) - at)
        t_in = cuda(stored[at:at + n])
        t_out = torch.zeros_like(t_in)
        poly.batch_inverse_device(F, t_in, n, t_out)
        got = host(t_out)
        assert all(v < p for v in O.array_to_ints(got)), (name, at)
        assert np.array_equal(got, want[at:at + n]), (name, at, [hex(vals[at + i]) for i in np.nonzero((got != want[at:at + n]).any(axis=1))[0][:4]])
    assert B % 256 == 0 and B > 256
    one = O.ints_to_array([R % p], 4)
    block_in, block_want = np.repeat(one, B, axis=0), np.repeat(one, B, axis=0)
    block_in[:256], block_want[:256] = stored[:256], want[:256]      # the edge set and the first powers of two
    t_in = cuda(block_in)
    t_out = torch.zeros_like(t_in)
    poly.batch_inverse_device(F, t_in, B, t_out)
    assert np.array_equal(host(t_out), block_want), name


@pytest.mark.parametrize("name", ["stark252", "fr381"])
def test_batch_inverse_reports_a_zero_element(name):
    from lambda_elliptic_curves_amd import errors, poly
    p, F = MODULI[name], fld(name)
    B, _sizes = inverse_sizes()
    stored = R2.to_stored(p, [v or 1 for v in rand_ints(p, 2 * B + 3, 5)])
    for n, at in ((2 * B + 3, B), (2 * B + 3, B + B // 2), (2 * B, 2 * B - 1), (1, 0), (2 * B + 3, 2 * B + 2)):
        a = stored[:n].copy()
        a[at] = 0
        with pytest.raises(errors.FieldError):
            poly.batch_inverse_device(F, cuda(a), n)
    with pytest.raises(errors.FieldError):
        poly.batch_inverse(F, np.zeros((3, 4), np.uint64))


# ---- constraint evaluations

def constraint_case(p, log2_trace, log2_blowup, offset, boundary, transitions, n_cols, seed):
    """random LDE columns and transition evaluations (the formula does not need a consistent trace)"""
    dom = R2.Domain(p, log2_trace, log2_blowup, offset)
    cols = [rand_ints(p, dom.N, seed + c) for c in range(n_cols)]
    tev = [rand_ints(p, dom.N, seed + 100 + c) for c in range(len(transitions))]
    return dom, cols, tev, R2.evaluate(dom, cols, boundary, transitions, tev)


def run_constraints(name, dom, cols, tev, boundary, transitions, log2_trace, log2_blowup, split_columns=False, stream=None):
    import torch
    from lambda_elliptic_curves_amd import stark
    p, F = MODULI[name], fld(name)
    if split_columns:      # separate allocations, as main and auxiliary tables are
        t_cols = [cuda(R2.to_stored(p, c)) for c in cols]
    else:
        t_all = cuda(R2.to_stored(p, [v for c in cols for v in c]).reshape(len(cols), dom.N, 4))
        t_cols = [t_all[c] for c in range(len(cols))]
    t_tev = cuda(R2.to_stored(p, [v for c in tev for v in c]).reshape(len(tev), dom.N, 4)) if tev else torch.zeros((1, 4), dtype=torch.int64, device="cuda")
    b, t = R2.stored_tables(p, boundary, transitions)
    t_out = stark.constraint_evaluations_device(F, t_cols, log2_trace, log2_blowup, R2.stored_one(p, dom.h), b, t, t_tev, stream=stream)
    return host(t_out)


RICH_TRANSITIONS = [
    dict(period=1, offset=0, end_exemptions=1, coeff=3),
    dict(period=1, offset=0, end_exemptions=1, coeff=5),                              # shares E and the cycle table with the first
    dict(period=4, offset=1, end_exemptions=0, coeff=7),
    dict(period=4, offset=1, end_exemptions=3, coeff=11),
    dict(period=4, offset=1, end_exemptions=1, exemptions_period=8, periodic_exemptions_offset=3, coeff=13),
    dict(period=1, offset=0, end_exemptions=0, exemptions_period=8, periodic_exemptions_offset=3, coeff=17),
]
RICH_BOUNDARY = [(0, 0, 1, 19), (2, 5, 12345, 23), (1, 0, 99, 29)]    # two distinct steps, column 2 is the auxiliary one

CONSTRAINT_SHAPES = {
    "golden_shape": (2, 2, [(0, 0, 1, 2), (0, 3, 3, 3)], [dict(period=1, end_exemptions=1, coeff=1), dict(period=1, end_exemptions=1, coeff=9)], 2),
    "n8_blowup2": (3, 1, [(1, 7, 4, 2)], [dict(period=2, offset=1, end_exemptions=1, coeff=6)], 2),
    "n64_blowup8_rich": (6, 3, RICH_BOUNDARY, RICH_TRANSITIONS, 3),
    "no_boundary": (6, 3, [], RICH_TRANSITIONS[:3], 1),
    "no_transitions": (6, 3, RICH_BOUNDARY, [], 3),
    "neither": (4, 1, [], [], 1),
    "cycle_as_long_as_N": (6, 2, [(0, 1, 2, 3)], [dict(period=64, offset=5, end_exemptions=1, coeff=4), dict(period=1, coeff=2)], 1),
    "five_steps": (4, 2, [(0, s, s + 1, s + 2) for s in (0, 3, 5, 8, 15)], [dict(period=1, end_exemptions=2, coeff=2)], 1),
    "N_2_13": (10, 3, RICH_BOUNDARY, RICH_TRANSITIONS[1:5], 3),
}


@pytest.mark.parametrize("shape", sorted(CONSTRAINT_SHAPES))
def test_constraint_evaluations_match_the_restatement(shape):
    log2_trace, log2_blowup, boundary, transitions, n_cols = CONSTRAINT_SHAPES[shape]
    p = MODULI["stark252"]
    dom, cols, tev, want = constraint_case(p, log2_trace, log2_blowup, 3, boundary, transitions, n_cols, 1000 + len(shape))
    got = run_constraints("stark252", dom, cols, tev, boundary, transitions, log2_trace, log2_blowup, split_columns=n_cols == 3)
    assert np.array_equal(got, R2.to_stored(p, want)), shape


def test_constraint_evaluations_stone_case_2_shape():
    """n = 512, blow-up 64: N = 2^15, the Fibonacci2ColsShifted constraint set"""
    p = MODULI["stark252"]
    boundary = [(0, 0, 1, 5), (0, 500, 77, 6)]
    transitions = [dict(period=1, end_exemptions=1, coeff=1), dict(period=1, end_exemptions=1, coeff=8)]
    dom, cols, tev, want = constraint_case(p, 9, 6, 3, boundary, transitions, 2, 41)
    got = run_constraints("stark252", dom, cols, tev, boundary, transitions, 9, 6)
    assert np.array_equal(got, R2.to_stored(p, want))


def test_constraint_evaluations_fr381():
    p = MODULI["fr381"]
    dom, cols, tev, want = constraint_case(p, 6, 3, 7, RICH_BOUNDARY, RICH_TRANSITIONS, 3, 51)
    got = run_constraints("fr381", dom, cols, tev, RICH_BOUNDARY, RICH_TRANSITIONS, 6, 3, split_columns=True)
    assert np.array_equal(got, R2.to_stored(p, want))


def test_constraint_evaluations_on_a_callers_stream():
    import torch
    p = MODULI["stark252"]
    log2_trace, log2_blowup, boundary, transitions, n_cols = CONSTRAINT_SHAPES["n64_blowup8_rich"]
    dom, cols, tev, want = constraint_case(p, log2_trace, log2_blowup, 3, boundary, transitions, n_cols, 61)
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    got = run_constraints("stark252", dom, cols, tev, boundary, transitions, log2_trace, log2_blowup, stream=s.cuda_stream)
    s.synchronize()
    assert np.array_equal(got, R2.to_stored(p, want))


def test_an_offset_inside_the_lde_group_is_a_zero_denominator():
    from lambda_elliptic_curves_amd import errors
    p = MODULI["stark252"]
    dom = R2.Domain(p, 3, 1, 1)
    for h in (1, dom.w, pow(dom.w, 5, p)):
        dom_h = R2.Domain(p, 3, 1, h)
        cols, tev = [rand_ints(p, dom.N, 1)], [rand_ints(p, dom.N, 2)]
        with pytest.raises(errors.FieldError):
            run_constraints("stark252", dom_h, cols, tev, [(0, 1, 2, 3)], [dict(period=1, coeff=1)], 3, 1)
    with pytest.raises(errors.FieldError):     # no boundary constraint: the zerofier's own denominator vanishes at x = 1
        run_constraints("stark252", dom, [rand_ints(p, dom.N, 1)], [rand_ints(p, dom.N, 2)], [], [dict(period=1, coeff=1)], 3, 1)


# ---- parts

@pytest.fixture(scope="module")
def part_inputs():
    """per log2_lde: (H canonical coefficients, their stored evaluations on the coset 3 <w>); H has non-zero coefficients
    up to the last one, beyond P n for every blow-up: the thinning case"""
    out = {}
    for log2_lde in (6, 13):
        H = rand_ints(D.P_STARK252, 1 << log2_lde, 900 + log2_lde)
        H[-1] = H[-2] = 0                 # so that the stripped lengths differ from the block lengths
        ev = O.evaluate_fft(O.F_STARK252, R2.to_stored(D.P_STARK252, H), 1, None, R2.stored_one(D.P_STARK252, 3))
        out[log2_lde] = (H, ev)
    return out


@pytest.mark.parametrize("log2_lde", [6, 13])
@pytest.mark.parametrize("n_parts", [1, 2, 3, 4])
def test_parts_match_break_in_parts_and_the_oracle_lde(part_inputs, log2_lde, n_parts):
    from lambda_elliptic_curves_amd import stark
    p, F = D.P_STARK252, fld("stark252")
    H, ev = part_inputs[log2_lde]
    off = R2.stored_one(p, 3)
    t_ev = cuda(ev)
    t_coeffs, lens, t_lde = stark.composition_parts_device(F, t_ev, log2_lde, off, n_parts)
    blocks, want_lens = R2.break_in_parts(H, n_parts)
    assert t_coeffs.shape == (n_parts, len(blocks[0]), 4) and lens == want_lens
    assert np.array_equal(host(t_coeffs), np.stack([R2.to_stored(p, b) for b in blocks]))
    assert np.array_equal(host(t_ev), ev)                                   # the input is left alone
    got_lde = host(t_lde)
    N, L = 1 << log2_lde, len(blocks[0])
    for j, b in enumerate(blocks):
        # evaluate_polynomial_on_lde_domain: the part's values at x_0 .. x_{N-1}
        want = O.evaluate_fft(O.F_STARK252, R2.to_stored(p, b), N // L, L, off)
        assert want.shape[0] == N and np.array_equal(got_lde[j], want), (n_parts, j)
    _c, no_lens, no_lde = stark.composition_parts_device(F, t_ev, log2_lde, off, n_parts, lde=False, lens=False)
    assert no_lens is None and no_lde is None and np.array_equal(host(_c), host(t_coeffs))


def test_parts_of_a_short_polynomial_and_fr381():
    from lambda_elliptic_curves_amd import stark
    p, F = D.P_FR381, fld("fr381")
    H = rand_ints(p, 5, 3) + [0] * 59
    off = R2.stored_one(p, 7)
    ev = O.evaluate_fft(O.F_FR381, R2.to_stored(p, H), 1, 64, off)
    t_coeffs, lens, t_lde = stark.composition_parts_device(F, cuda(ev), 6, off, 3)
    blocks, want_lens = R2.break_in_parts(H, 3)
    assert lens == want_lens == [2, 2, 1]
    assert np.array_equal(host(t_coeffs), np.stack([R2.to_stored(p, b) for b in blocks]))
    for j, b in enumerate(blocks):
        assert np.array_equal(host(t_lde)[j], O.evaluate_fft(O.F_FR381, R2.to_stored(p, b), 2, 32, off))


# ---- commitment

@pytest.mark.parametrize("log2_leaves,n_parts", [(3, 1), (3, 3), (9, 2), (10, 2), (13, 3), (17, 2)])
def test_composition_commitment_matches_the_oracle_tree(log2_leaves, n_parts):
    """2^3: the top kernel only; 2^10, 2^13: levels fused into the leaf kernel; 2^17: 16 x 16 leaf tiles, a launch per
    wide level"""
    import torch
    from lambda_elliptic_curves_amd import merkle
    F, log2_lde = fld("stark252"), log2_leaves + 1
    N = 1 << log2_lde
    parts = util.rand_elems("stark252", n_parts * N, 40 + log2_leaves).reshape(n_parts, N, 4)
    t_nodes = torch.zeros((N - 1) * 4, dtype=torch.int64, device="cuda")
    root = merkle.commit_composition_device(F, cuda(parts), n_parts, log2_lde, t_nodes)
    want = R2.composition_nodes(parts)
    got = host(t_nodes).view(np.uint8).reshape(-1, 32)
    assert got.shape == want.shape and np.array_equal(got, want)
    assert root == bytes(want[0])
    if log2_leaves == 3:
        assert np.array_equal(want, R2.composition_nodes_by_rows(parts))


def test_composition_commitment_with_a_column_stride():
    import torch
    from lambda_elliptic_curves_amd import merkle
    F, log2_lde, n_parts = fld("stark252"), 10, 2
    N, stride = 1 << log2_lde, (1 << log2_lde) + 24
    buf = util.rand_elems("stark252", n_parts * stride, 9).reshape(n_parts, stride, 4)
    t_nodes = torch.zeros((N - 1) * 4, dtype=torch.int64, device="cuda")
    root = merkle.commit_composition_device(F, cuda(buf), n_parts, log2_lde, t_nodes, col_stride_elems=stride)
    want = R2.composition_nodes(buf[:, :N])
    assert np.array_equal(host(t_nodes).view(np.uint8).reshape(-1, 32), want) and root == bytes(want[0])


# ---- end to end: Stone-compatibility case 1

def test_round2_reproduces_the_stone_compat_commitment_and_feeds_rounds_3_and_4():
    import torch
    from lambda_elliptic_curves_amd import fft, poly, stark
    with open(os.path.join(ROOT, "tests", "golden", "stark_round2.json")) as f:
        golden = json.load(f)
    p, F = D.P_STARK252, fld("stark252")
    log2_trace, log2_blowup, n_parts = golden["log2_trace"], golden["log2_blowup"], golden["n_parts"]
    log2_lde = log2_trace + log2_blowup
    n, N = 1 << log2_trace, 1 << log2_lde
    off = R2.stored_one(p, golden["coset_offset"])
    beta = int(golden["beta"], 16)
    # round 1 on the device: interpolate the trace, extend it to the LDE coset
    trace = np.stack([R2.to_stored(p, c) for c in util.stone_compat_trace_columns(int(golden["trace_initial"], 16), n)])
    t_trace = cuda(trace)
    t_polys = torch.empty_like(t_trace)
    fft.ntt_device(F, t_trace, t_polys, log2_trace, inverse=True, batch=2)
    t_lde = torch.empty((2, N, 4), dtype=torch.int64, device="cuda")
    fft.lde_device(F, t_polys, log2_trace, t_lde, log2_lde, batch=2, offset=off)
    # the AIR's compute_transition, on the host from the downloaded 16 rows
    lde = [R2.from_stored(p, c) for c in host(t_lde)]
    dom = R2.Domain(p, log2_trace, log2_blowup, golden["coset_offset"])
    t0 = [(lde[0][R2.frame_row(dom, i, 1)] - lde[1][i]) % p for i in range(N)]
    t1 = [(lde[1][R2.frame_row(dom, i, 1)] - lde[0][i] - lde[1][i]) % p for i in range(N)]
    tev = np.stack([R2.to_stored(p, t0), R2.to_stored(p, t1)])
    boundary, transitions = R2.stored_tables(p, [(0, 0, 1, pow(beta, 2, p)), (0, 3, 3, pow(beta, 3, p))],
                                            [dict(period=1, end_exemptions=1, coeff=1), dict(period=1, end_exemptions=1, coeff=beta)])
    t_cols = [t_lde[0], t_lde[1]]
    t_parts, lens, t_parts_lde, t_nodes, root = stark.round2_device(F, t_cols, log2_trace, log2_blowup, off, boundary, transitions,
                                                                    cuda(tev), n_parts)
    assert root.hex() == golden["composition_root"]
    z = R2.stored_one(p, int(golden["z"], 16))
    assert R2.from_stored(p, poly.evaluate_device(F, t_parts, lens, z.reshape(1, 4))[0, 0]) == [int(golden["h0_at_z"], 16)]
    # the host form returns the same bytes
    h_coeffs, h_lens, h_root, h_nodes, h_lde = stark.round2(F, host(t_lde), log2_trace, log2_blowup, off, boundary, transitions, tev,
                                                            n_parts, return_nodes=True, return_lde=True)
    assert h_root == root and h_lens == lens
    assert np.array_equal(h_coeffs, np.stack([host(t) for t in t_parts]))
    assert np.array_equal(h_lde, host(t_parts_lde))
    assert np.array_equal(h_nodes, host(t_nodes).view(np.uint8).reshape(-1, 32))
    # round 3 / the DEEP composition polynomial takes the parts as they are
    g = R2.stored_one(p, dom.g)
    gamma = R2.stored_one(p, 0x1234567)
    t_deep = torch.empty((max(n, max(lens)) - 1, 4), dtype=torch.int64, device="cuda")
    _deep_len, _trace_ood, parts_ood = stark.deep_composition_poly_device(F, [t_polys[0], t_polys[1]], [n, n], t_parts, lens, z, g, 2, gamma, t_deep)
    assert R2.from_stored(p, parts_ood[0]) == [int(golden["h0_at_z"], 16)]   # z^P = z for one part
    # round 4's openings on the real tree fold to the committed root
    iotas = [0, 3, N // 2 - 1]
    main_nodes = torch.empty((2 * N - 1) * 4, dtype=torch.int64, device="cuda")
    from lambda_elliptic_curves_amd import merkle
    merkle.commit_columns_device(F, t_lde, 2, log2_lde, main_nodes)
    opened = stark.open_deep_composition_poly_device(F, (t_lde, 2, log2_lde, main_nodes), (t_parts_lde, n_parts, log2_lde, t_nodes), iotas)
    parts_host = host(t_parts_lde)
    for entry, iota in zip(opened, iotas):
        comp = entry["composition"]
        want = Q.open_composition_poly(parts_host, h_nodes, log2_lde, iota)
        assert np.array_equal(comp["evaluations"], want["evaluations"]) and np.array_equal(comp["evaluations_sym"], want["evaluations_sym"])
        leaf = b"".join(int(w).to_bytes(8, "big") for w in np.concatenate([comp["evaluations"], comp["evaluations_sym"]]).reshape(-1))
        assert Q.fold_path(O.keccak256(leaf), iota, comp["proof"]) == root
