"""Circle STARK round 2 over Mersenne31 with QM31 on the device (csrc/circle_round2.cuh) against the model of
tests/circle_round2_ref.py, bit for bit: the fused constraint evaluations (the AIR's program, the zerofiers of doubled points,
the end-exemption lines, the random linear combination in QM31, the boundary quotients), the parts of the composition
polynomial as index blocks, their Monolith commitment, the prover's own identity at a point of the circle over QM31 and the
chain from the LDE to a constant last FRI layer.

Launch boundaries (the constants of circle_round2.cuh): the transition kernel gives a work-item one LDE row and a block 256;
the boundary kernel gives a work-item M31Q_R2_ROWS = 4 rows (a block 1024) and a launch M31Q_R2_STEPS = 4 distinct steps; a
call takes M31Q_R2_CLASSES = 8 distinct transition zerofiers; a cycle work-item takes 4 entries."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from lambda_elliptic_curves_amd import _lib as L
from lambda_elliptic_curves_amd import circle, errors, fft, merkle, monolith, stark
from lambda_elliptic_curves_amd import mersenne31_ext as E
from tests import air_program_ref as A
from tests import circle_ref as CR
from tests import circle_round2_ref as M
from tests import mersenne31_ext_ref as R
from tests import monolith_ref as MR

pytestmark = pytest.mark.gpu
P = M.P
EDGE = [0, 1, P - 1, P, 1 << 31, (1 << 32) - 1]
R2_ROWS, R2_STEPS, R2_CLASSES = 4, 4, 8
ROUNDS = 5
MARK = 0x5A5A5A5A


def dev(a):
    return torch.from_numpy(np.array(a, dtype=np.uint32, order="C").view(np.int32).reshape(-1)).cuda()


def host(t):
    return t.cpu().numpy().view(np.uint32)


def rand_elems(n, seed):
    return [tuple(int(v) for v in row) for row in np.random.default_rng(seed).integers(0, P, (n, 4))]


def rand_words(n, seed, values=None):
    rng = np.random.default_rng(seed)
    if values:
        return [values[int(k)] for k in rng.integers(0, len(values), n)]
    return [int(v) for v in rng.integers(0, P, n)]


def program_of(ops, n_transitions):
    return stark.AirProgram(np.array(ops, dtype=stark.AIR_OP_DTYPE), n_transitions)


def elems_of(t, n, stride=0):
    stride = stride or n
    h = host(t).reshape(-1)
    return [tuple(int(h[e * stride + i]) for e in range(4)) for i in range(n)]


def device_call(dom, raw_cols, program, consts, boundary, transitions, lens=None, t_out=None, out_stride=0):
    """words as they go to the device (any u32) -> the N elements of out"""
    t_cols = [dev(c) for c in raw_cols]
    t = E.constraint_evaluations_device(program, consts, t_cols, dom.log2_trace, dom.log2_blowup, boundary, transitions, t_out=t_out, out_stride=out_stride,
                                        col_log2_len=lens)
    return elems_of(t, dom.N, out_stride)


def model_call(dom, raw_cols, program, consts, boundary, transitions):
    cols = [[CR.reduce_word(w) for w in c] for c in raw_cols]
    bnd = [(col, step, CR.reduce_word(value), R.elem(coeff)) for col, step, value, coeff in boundary]
    trs = [dict(t, coeff=R.elem(t["coeff"])) for t in transitions]
    return M.evaluate(dom, cols, program.ops.tolist(), [CR.reduce_word(c) for c in consts], bnd, trs)


def check(dom, raw_cols, program, consts, boundary, transitions, **kw):
    assert device_call(dom, raw_cols, program, consts, boundary, transitions, **kw) == model_call(dom, raw_cols, program, consts, boundary, transitions)


def air_inputs(name, log2_trace, log2_blowup, seed, values=None):
    """-> (dom, columns (a periodic one short), col_log2_len or None, constants, program)"""
    build, n_cols, n_consts, periodic = A.AIRS[name]
    dom = M.Domain(log2_trace, log2_blowup)
    lens = [periodic[c] * dom.blowup if c in periodic else dom.N for c in range(n_cols)]
    cols = [rand_words(ln, seed + c, values) for c, ln in enumerate(lens)]
    consts = rand_words(n_consts, seed + 50, values)
    return dom, cols, ([ln.bit_length() - 1 for ln in lens] if periodic else None), consts, stark.compile_transitions(build(stark))


def descriptors(n_transitions, seed, end_exemptions=1):
    coeffs = rand_elems(n_transitions, seed)
    return [dict(period=1, offset=0, end_exemptions=end_exemptions + c % 2, coeff=coeffs[c]) for c in range(n_transitions)]


# ---- the example AIRs
@pytest.mark.parametrize("shape", [(3, 2), (8, 2)], ids=["one_block", "several_blocks"])
@pytest.mark.parametrize("air", sorted(A.AIRS))
def test_example_airs(air, shape):
    dom, cols, lens, consts, program = air_inputs(air, shape[0], shape[1], 11)
    gammas = rand_elems(2, 12)
    boundary = [(0, 0, 5, gammas[0]), (0, dom.n - 1, 7, gammas[1])]
    check(dom, cols, program, consts, boundary, descriptors(program.n_transitions, 13), lens=lens)


# ---- the zerofier, one branch at a time: one transition with coefficient 1, no boundary (n = 16)
ZEROFIERS = {
    "no_exemptions": dict(period=1, offset=0, end_exemptions=0),
    "one_exemption": dict(period=1, offset=0, end_exemptions=1),
    "two_exemptions": dict(period=1, offset=0, end_exemptions=2),
    "period_2_offset_1": dict(period=2, offset=1, end_exemptions=1),
    "period_half_the_trace": dict(period=8, offset=3, end_exemptions=1),      # m = 2: no doubling
    "every_row_exempt": dict(period=4, offset=2, end_exemptions=4),           # end_exemptions = n / period
}


@pytest.mark.parametrize("branch", sorted(ZEROFIERS))
def test_zerofier_branches(branch):
    dom, cols, lens, consts, program = air_inputs("quadratic", 4, 2, 21)
    check(dom, cols, program, consts, [], [dict(ZEROFIERS[branch], coeff=(1, 0, 0, 0))])


def test_identical_descriptors_share_a_class():
    dom, cols, lens, consts, program = air_inputs("rom", 4, 2, 22)
    same, other = dict(period=2, offset=1, end_exemptions=1), dict(period=1, offset=0, end_exemptions=2)
    coeffs = rand_elems(3, 23)
    check(dom, cols, program, consts, [], [dict(same, coeff=coeffs[0]), dict(other, coeff=coeffs[1]), dict(same, coeff=coeffs[2])])


def many_constraints(n):
    return stark.compile_transitions([stark.cell(0, 1 + k % 3) - stark.cell(0) for k in range(n)])


def test_descriptor_cap():
    dom = M.Domain(5, 2)
    cols = [rand_words(dom.N, 24)]
    coeffs = rand_elems(R2_CLASSES + 1, 25)
    full = [dict(period=1 << (c % 3), offset=c % (1 << (c % 3)), end_exemptions=c, coeff=coeffs[c]) for c in range(R2_CLASSES)]
    assert len({(t["period"], t["offset"], t["end_exemptions"]) for t in full}) == R2_CLASSES
    check(dom, cols, many_constraints(R2_CLASSES), [], [], full)
    with pytest.raises(errors.HipError, match="distinct transition zerofiers"):
        device_call(dom, cols, many_constraints(R2_CLASSES + 1), [], [], full + [dict(period=1, offset=0, end_exemptions=R2_CLASSES, coeff=coeffs[-1])])
    # a ninth transition that shares a descriptor is no ninth class
    check(dom, cols, many_constraints(R2_CLASSES + 1), [], [], full + [dict(full[3], coeff=coeffs[-1])])


# ---- the boundary part
@pytest.mark.parametrize("n_steps", [1, 4, 5, 9])
def test_boundary_step_groups(n_steps):
    dom, cols, lens, consts, program = air_inputs("fib2", 4, 2, 31)
    g = rand_elems(n_steps + 3, 32 + n_steps)
    steps = [5, 0, 9, dom.n - 1, 2, 7, 15 - 4, 1, 8][:n_steps]
    many = [(k % 2, step, 3 + k, g[k]) for k, step in enumerate(steps)]
    many += [(1, steps[0], P - 1, g[-1]), (0, steps[-1], 0, g[-2]), (1, steps[0], 9, g[-3])]      # several constraints on one step
    assert len({s for _, s, _, _ in many}) == n_steps
    trs = descriptors(2, 33)
    check(dom, cols, program, consts, many, trs)
    check(dom, cols, program_of([], 0), consts, many, [])            # n_transitions = 0: the program is empty too


def test_no_boundary_and_nothing_at_all():
    dom, cols, lens, consts, program = air_inputs("fib2", 3, 2, 34)
    check(dom, cols, program, consts, [], descriptors(2, 35))
    t_out = dev([1] * (4 * dom.N))
    assert device_call(dom, cols, program_of([], 0), [], [], [], t_out=t_out) == [R.ZERO] * dom.N


@pytest.mark.parametrize("log2_trace", [7, 8, 9], ids=["below", "at", "above"])
def test_rows_around_one_boundary_block(log2_trace):
    """N = 512, 1024, 2048 against the R x 256 = 1024 rows of a boundary block"""
    dom = M.Domain(log2_trace, 2)
    assert (dom.N < R2_ROWS * 256, dom.N == R2_ROWS * 256, dom.N > R2_ROWS * 256) == (log2_trace == 7, log2_trace == 8, log2_trace == 9)
    cols = [rand_words(dom.N, 36 + c) for c in range(2)]
    g = rand_elems(3, 38)
    check(dom, cols, program_of([], 0), [], [(0, 0, 1, g[0]), (1, dom.n - 1, 2, g[1]), (1, dom.n // 2 + 1, 3, g[2])], [])


# ---- operands at the edges
@pytest.mark.parametrize("air", ["rom", "fib_rap", "periodic"])
def test_edge_words_in_cells_constants_values_and_coefficients(air):
    dom, cols, lens, consts, program = air_inputs(air, 4, 2, 41, values=EDGE)
    assert all(set(EDGE) <= set(c) for c in cols if len(c) == dom.N)
    coeffs = [tuple(EDGE[(k + e) % 6] for e in range(4)) for k in range(6)]
    trs = [dict(period=1, offset=0, end_exemptions=1, coeff=coeffs[c]) for c in range(program.n_transitions)]
    boundary = [(0, k, EDGE[k], coeffs[5 - k]) for k in range(6)]
    check(dom, cols, program, consts, boundary, trs, lens=lens)


def test_all_eight_temporaries():
    dom = M.Domain(5, 2)
    cols = [rand_words(dom.N, 45 + c) for c in range(2)]
    program = stark.compile_transitions([A.all_temporaries(stark)])
    assert program.n_tmps == A.MAX_TMPS
    check(dom, cols, program, [], [(1, 2, 9, rand_elems(1, 47)[0])], descriptors(1, 48))


def test_program_of_the_maximal_length():
    dom = M.Domain(4, 1)
    cols = [rand_words(dom.N, 49 + c) for c in range(2)]
    ops = [(A.LOAD, A.CELL, 0, 0)] + [((A.ADD, A.MUL, A.SUB)[k % 3], A.CELL, k % 2, k % dom.n) for k in range(A.MAX_OPS - 2)] + [(A.EMIT, 0, 0, 0)]
    assert len(ops) == A.MAX_OPS
    check(dom, cols, program_of(ops, 1), [], [], descriptors(1, 51))


# ---- the output's stride
def test_out_stride_leaves_the_gaps_untouched():
    dom, cols, lens, consts, program = air_inputs("fib2", 4, 2, 61)
    stride = dom.N + 8
    t_out = dev([MARK] * (4 * stride + 8))
    boundary, trs = [(0, 0, 1, rand_elems(1, 62)[0])], descriptors(2, 63)
    got = device_call(dom, cols, program, consts, boundary, trs, t_out=t_out, out_stride=stride)
    assert got == model_call(dom, cols, program, consts, boundary, trs)
    words = host(t_out)
    assert (words[:4 * stride].reshape(4, stride)[:, dom.N:] == MARK).all() and (words[4 * stride:] == MARK).all()


# ---- the parts
@functools.lru_cache(maxsize=None)
def parts_case(broken):
    """a composition polynomial of 2^6 coefficients a plane: 24 of them non-zero, or all of them"""
    dom = M.Domain(4, 2)
    live = dom.N if broken else 24
    H = [rand_words(live, 71 + e) + [0] * (dom.N - live) for e in range(4)]
    planes = [CR.evaluate_cfft(h) for h in H]
    evals = [tuple(planes[e][i] for e in range(4)) for i in range(dom.N)]
    return dom, H, evals


def parts_call(dom, evals, log2_part, n_parts, lde=True, tail=True, evals_stride=0):
    """through the C entry, with guard words behind both outputs -> (coeff planes, LDE planes or None, tail, the evaluations after the call)"""
    Lw, planes = 1 << log2_part, 4 * n_parts
    stride = evals_stride or dom.N
    ev = np.full(4 * stride, MARK, np.uint32)
    for e in range(4):
        ev[e * stride: e * stride + dom.N] = [v[e] for v in evals]
    t_ev = dev(ev)
    t_coeffs, t_lde = dev([MARK] * (planes * Lw + 8)), dev([MARK] * (planes * dom.N + 8))
    count = C.c_uint64(12345)
    errors.check(L.lib().lw_mersenne31_ext4_composition_parts_device(L.device_ptr(t_ev), evals_stride, dom.log2_lde, log2_part, n_parts, L.device_ptr(t_coeffs),
                                                                    L.device_ptr(t_lde) if lde else None, C.byref(count) if tail else None, None))
    torch.cuda.synchronize()
    c, l = host(t_coeffs), host(t_lde)
    assert (c[planes * Lw:] == MARK).all() and (l[planes * dom.N if lde else 0:] == MARK).all()
    assert np.array_equal(host(t_ev), ev)                                  # d_evals is not modified
    return c[:planes * Lw].reshape(planes, Lw).tolist(), (l[:planes * dom.N].reshape(planes, dom.N).tolist() if lde else None), (count.value if tail else None)


@pytest.mark.parametrize("shape", [(6, 1), (5, 2), (4, 4), (3, 8), (5, 1), (4, 2), (3, 4), (2, 8)], ids=lambda s: "L%d_P%d" % (1 << s[0], s[1]))
def test_composition_parts(shape):
    log2_part, n_parts = shape
    dom, H, evals = parts_case(False)
    coeffs, lde, tail = parts_call(dom, evals, log2_part, n_parts)
    want_coeffs, want_lde, want_tail = M.parts(dom, evals, log2_part, n_parts)
    assert coeffs == want_coeffs and lde == want_lde and tail == want_tail == 0       # 24 <= P L = 32 or 64
    Lw = 1 << log2_part
    assert coeffs == [H[e][j * Lw:(j + 1) * Lw] for j in range(n_parts) for e in range(4)]
    dom, H, evals = parts_case(True)                                                    # every coefficient alive
    coeffs, lde, tail = parts_call(dom, evals, log2_part, n_parts)
    want_coeffs, want_lde, want_tail = M.parts(dom, evals, log2_part, n_parts)
    assert coeffs == want_coeffs and lde == want_lde and tail == want_tail
    assert tail == sum(1 for e in range(4) for w in H[e][n_parts * Lw:] if w) and (tail > 0) == (n_parts * Lw < dom.N)


def test_composition_parts_without_lde_without_tail_and_under_a_stride():
    dom, H, evals = parts_case(True)
    want_coeffs, want_lde, want_tail = M.parts(dom, evals, 4, 2)
    assert parts_call(dom, evals, 4, 2, lde=False) == (want_coeffs, None, want_tail)
    assert parts_call(dom, evals, 4, 2, tail=False) == (want_coeffs, want_lde, None)
    assert parts_call(dom, evals, 4, 2, evals_stride=dom.N + 12) == (want_coeffs, want_lde, want_tail)
    # the wrapper
    t_ev = dev([[v[e] for v in evals] for e in range(4)])
    t_coeffs, t_lde, tail = E.composition_parts_device(t_ev, dom.log2_lde, 4, 2, tail=True)
    assert host(t_coeffs).reshape(8, 16).tolist() == want_coeffs and host(t_lde).reshape(8, dom.N).tolist() == want_lde and tail == want_tail
    t_coeffs, t_lde, tail = E.composition_parts_device(t_ev, dom.log2_lde, 4, 2, lde=False)
    assert host(t_coeffs).reshape(8, 16).tolist() == want_coeffs and t_lde is None and tail is None


# ---- the prover's own identity, the low degree, the commitment and the chain
def valid_trace(air, n):
    if air == "quadratic":
        a = [3]
        for _ in range(n - 1):
            a.append(a[-1] * a[-1] % P)
        return [a], {}
    a = [1, 1]
    for _ in range(n - 2):
        a.append((a[-1] + a[-2]) % P)
    return [a, [7, P - 2]], {1: 2}      # simple_periodic_cols: s (a'' - a' - a), s of period 2


@functools.lru_cache(maxsize=None)
def round2_case(air, broken=False):
    """a trace of 2^4 rows that satisfies the AIR (or has one cell changed), blow-up 4: LDE on the device -> the evaluations"""
    dom = M.Domain(4, 2)
    trace, periodic = valid_trace(air, dom.n)
    if broken:
        trace[0][6] = (trace[0][6] + 1) % P
    t_trace = dev(trace[0])
    t_col = torch.zeros(dom.N, dtype=torch.int32, device="cuda")
    circle.lde_device(t_trace, dom.log2_trace, t_col, dom.log2_lde)
    t_cols, lens, polys = [t_col], None, [CR.interpolate_cfft(trace[0])]
    if periodic:                                                         # the short column: the period's polynomial on the coset of 2 B points
        polys.append(CR.interpolate_cfft(trace[1]))
        t_cols.append(dev(CR.evaluate_cfft(polys[1] + [0] * (2 * dom.blowup - 2))))
        lens = [dom.log2_lde, 1 + dom.log2_blowup]
    program = stark.compile_transitions(A.AIRS[air][0](stark))
    coeffs = rand_elems(3, 81)
    exemptions = 1 if air == "quadratic" else 2
    transitions = [dict(period=1, offset=0, end_exemptions=exemptions, coeff=coeffs[0])]
    boundary = [(0, 0, trace[0][0], coeffs[1]), (0, dom.n - 1, trace[0][-1], coeffs[2])]
    assert M.degree_bound(dom, 2, exemptions) == 32
    return dom, trace, polys, t_cols, lens, program, boundary, transitions


@pytest.mark.parametrize("air", ["quadratic", "periodic"])
def test_the_provers_identity_at_a_point_of_the_circle(air):
    dom, trace, polys, t_cols, lens, program, boundary, transitions = round2_case(air)
    log2_part, n_parts = 4, 2                                            # P L = 32: the bound of lw_hip.h for degree 2
    t_coeffs, t_lde, t_nodes, root = E.round2_device(program, [], t_cols, dom.log2_trace, dom.log2_blowup, boundary, transitions, log2_part, n_parts, ROUNDS,
                                                     col_log2_len=lens)
    z = R.circle_point(rand_elems(1, 82)[0])
    assert R.add(R.sqr(z[0]), R.sqr(z[1])) == R.ONE
    rows = [0, 1, 2]
    pts = M.frame_points(dom, z, rows)
    at = E.evaluate_device(dev(polys[0]), 1, dom.log2_trace, pts)
    cells = {(0, r): tuple(int(x) for x in at[0, k]) for k, r in enumerate(rows)}
    assert cells[(0, 1)] == R.evaluate(polys[0], pts[1])
    if air == "periodic":
        at = E.evaluate_device(dev(polys[1]), 1, 1, [M.periodic_point(dom, 2, pt) for pt in pts])
        cells.update({(1, r): tuple(int(x) for x in at[0, k]) for k, r in enumerate(rows)})
    want = M.composition_at(dom, lambda col, row: cells[(col, row)], program.ops.tolist(), [], boundary, transitions, z)
    Lw = 1 << log2_part
    factors = E.part_factors(z, log2_part, n_parts)
    assert factors == M.part_factors(z, log2_part, n_parts)
    total = R.ZERO
    for j in range(n_parts):
        hj = E.evaluate_ext_device(t_coeffs[4 * j * Lw: 4 * (j + 1) * Lw], log2_part, [z])[0]
        total = R.add(total, R.mul(factors[j], hj))
    assert total == want and want != R.ZERO


def test_low_degree_through_the_chain():
    for broken in (False, True):
        dom, trace, polys, t_cols, lens, program, boundary, transitions = round2_case("quadratic", broken)
        t_ev = E.constraint_evaluations_device(program, [], t_cols, dom.log2_trace, dom.log2_blowup, boundary, transitions)
        model = M.evaluate(dom, [host(t_cols[0]).tolist()], program.ops.tolist(), [], boundary, transitions)
        assert elems_of(t_ev, dom.N) == model
        t_H = torch.zeros_like(t_ev)
        circle.interpolate_cfft_device(t_ev, t_H, dom.log2_lde, batch=4)
        H = host(t_H).reshape(4, dom.N)
        last = max(int(np.flatnonzero(H.any(axis=0))[-1]), -1)
        assert last == M.last_nonzero(model)
        bound = M.degree_bound(dom, 2, 1)
        assert bound == 32 and (last >= bound) == broken
        assert E.composition_parts_device(t_ev, dom.log2_lde, 4, 2, lde=False, tail=True)[2] == int(np.count_nonzero(H[:, bound:]))
        assert last == (63 if broken else 18)


def bitrev(i, bits):
    return int(format(i, "0%db" % bits)[::-1], 2)


def test_round2_commits_the_planes_of_the_parts_and_one_opening_verifies():
    dom, trace, polys, t_cols, lens, program, boundary, transitions = round2_case("quadratic")
    t_coeffs, t_lde, t_nodes, root = E.round2_device(program, [], t_cols, dom.log2_trace, dom.log2_blowup, boundary, transitions, 4, 2, ROUNDS)
    model = M.evaluate(dom, [host(t_cols[0]).tolist()], program.ops.tolist(), [], boundary, transitions)
    want_coeffs, want_lde, tail = M.parts(dom, model, 4, 2)
    assert tail == 0 and host(t_coeffs).reshape(8, 16).tolist() == want_coeffs and host(t_lde).reshape(8, dom.N).tolist() == want_lde
    planes = np.array(want_lde, np.uint32)
    assert np.array_equal(root, monolith.commit_columns(ROUNDS, planes))
    nodes = MR.np_tree(ROUNDS, planes, True)
    assert np.array_equal(host(t_nodes).reshape(-1, 8), nodes) and np.array_equal(root, nodes[0])
    pos = 37
    _, paths = merkle.open_trees_device([merkle.Tree(fft.Stark252PrimeField, t_nodes, dom.log2_lde)], np.array([[pos]], np.uint64))
    cur = MR.hash(ROUNDS, [int(x) for x in planes[:, bitrev(pos, dom.log2_lde)]])
    assert cur == nodes[dom.N - 1 + pos].tolist()
    i = pos
    for sib in paths[0][0].view(np.uint32).reshape(-1, 8).tolist():
        cur = MR.compress(ROUNDS, cur, sib) if i % 2 == 0 else MR.compress(ROUNDS, sib, cur)
        i >>= 1
    assert cur == nodes[0].tolist()


def transcript(prev):
    seed = 7 if prev is None else int(np.asarray(prev, np.uint64).sum() % P)
    return (seed, (seed * 3 + 1) % P, (seed * 5 + 2) % P, (seed * 7 + 3) % P)


def test_chain_from_the_lde_through_round_2_to_a_constant_last_layer():
    """circle.lde_device -> round2_device -> evaluate_device -> deep_quotients_device -> fri_commit_phase_device: the trace
    column and the eight planes of the two parts have 2^4 coefficients each, so four folds of the DEEP vector leave a constant"""
    dom, trace, polys, t_cols, lens, program, boundary, transitions = round2_case("quadratic")
    log2_part, n_parts = 4, 2
    t_coeffs, t_lde, t_nodes, root = E.round2_device(program, [], t_cols, dom.log2_trace, dom.log2_blowup, boundary, transitions, log2_part, n_parts, ROUNDS)
    z = R.circle_point(rand_elems(1, 91)[0])
    n_cols = 1 + 4 * n_parts
    t_all_coeffs = torch.cat([dev(polys[0]), t_coeffs])                   # 9 columns of 2^4 coefficients
    v = E.evaluate_device(t_all_coeffs, n_cols, dom.log2_trace, [z])
    evals = [[tuple(int(x) for x in v[k, 0])] for k in range(n_cols)]
    w = rand_elems(1 + n_parts, 92)
    weights = [[w[0]]] + [row for j in range(n_parts) for row in E.plane_weights([w[1 + j]])]
    t_all_lde = torch.cat([t_cols[0], t_lde])
    t_deep = torch.zeros(4 * dom.N, dtype=torch.int32, device="cuda")
    E.deep_quotients_device(t_all_lde, n_cols, dom.log2_lde, [z], weights, evals, t_deep)
    last, layers = E.fri_commit_phase_device(t_deep, dom.log2_lde, dom.log2_trace, ROUNDS, transcript)
    assert len(last) == 4 and last[0] == last[1] == last[2] == last[3] and last[0] != R.ZERO
    assert len(layers) == dom.log2_trace - 1
    # with one claimed value wrong the last layer is no constant
    evals[3] = [R.add(evals[3][0], R.ONE)]
    E.deep_quotients_device(t_all_lde, n_cols, dom.log2_lde, [z], weights, evals, t_deep)
    last, _ = E.fri_commit_phase_device(t_deep, dom.log2_lde, dom.log2_trace, ROUNDS, transcript)
    assert not last[0] == last[1] == last[2] == last[3]
