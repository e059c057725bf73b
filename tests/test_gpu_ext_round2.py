"""STARK round 2 over Goldilocks with Fp2 and over BabyBear with Fp4 on the device (csrc/ext_round2.cuh) against the model of
tests/ext_round2_ref.py, bit for bit: the fused constraint evaluations (the AIR's program, the zerofiers, the random linear
combination in the extension, the boundary quotients), the parts of the composition polynomial, their commitment and the
prover's own check at an out-of-domain point.

Launch boundaries (the constants of ext_round2.cuh): the transition kernel gives a work-item one LDE row and a block 256;
the boundary kernel gives a work-item EXT_ROWS = 4 rows and a launch EXT_R2_STEPS = 4 distinct steps; a call takes
EXT_R2_CLASSES = 8 distinct transition zerofiers."""
import functools

import numpy as np
import pytest
import torch

from lambda_elliptic_curves_amd import babybear_ext, errors, fft, goldilocks, goldilocks_ext, merkle, rpo, stark
from tests import air_program_ref as A
from tests import ext_round2_ref as M

pytestmark = pytest.mark.gpu
FIELDS = ["gl2", "bb4"]
R2_STEPS, R2_CLASSES = 4, 8
MOD = {"gl2": goldilocks_ext, "bb4": babybear_ext}
NP = {"gl2": np.uint64, "bb4": np.uint32}
TORCH = {"gl2": torch.int64, "bb4": torch.int32}
SIGNED = {"gl2": np.int64, "bb4": np.int32}


def dev(name, words):
    return torch.from_numpy(np.array(words, dtype=NP[name], order="C").view(SIGNED[name])).cuda()


def host(name, t):
    return t.cpu().numpy().view(NP[name])


def rand_elems(F, n, seed):
    rng = np.random.default_rng(seed)
    return [tuple(int.from_bytes(rng.bytes(16), "big") % F.p for _ in range(F.width)) for _ in range(n)]


def program_of(ops, n_transitions):
    return stark.AirProgram(np.array(ops, dtype=stark.AIR_OP_DTYPE), n_transitions)


def device_call(F, dom, cols, program, consts, boundary, transitions, lens=None, raw_cols=None, t_out=None, out_stride=0):
    """canonical inputs (raw_cols: the words of the columns as they go to the device) -> the N elements of E, canonical"""
    name, log2_trace = F.name, dom.n.bit_length() - 1
    t_cols = [dev(name, raw_cols[k] if raw_cols else [F.word(v) for v in c]) for k, c in enumerate(cols)]
    bnd = [(col, step, F.word(value), F.word_elem(coeff)) for col, step, value, coeff in boundary]
    trs = [dict(t, coeff=F.word_elem(t["coeff"])) for t in transitions]
    t = MOD[name].constraint_evaluations_device(program, [F.word(c) for c in consts], t_cols, log2_trace, dom.log2_lde - log2_trace, bnd, trs, t_out=t_out,
                                                out_stride=out_stride, offset=F.word(dom.h), col_log2_len=lens)
    stride = out_stride or dom.N
    planes = host(name, t)
    return [tuple(F.unword(planes[e * stride + i]) for e in range(F.width)) for i in range(dom.N)]


def check(F, dom, cols, program, consts, boundary, transitions, **kw):
    got = device_call(F, dom, cols, program, consts, boundary, transitions, **kw)
    want = M.evaluate(F, dom, cols, program.ops.tolist(), consts, boundary, transitions)
    assert got == want


def air_inputs(F, name, log2_trace, log2_blowup, seed, values=None):
    """-> (dom, canonical columns (a periodic one short), col_log2_len or None, constants, program)"""
    build, n_cols, n_consts, periodic = A.AIRS[name]
    dom = M.domain(F, log2_trace, log2_blowup, 3)
    lens = [periodic[c] * dom.blowup if c in periodic else dom.N for c in range(n_cols)]
    rng = np.random.default_rng(seed)
    draw = (lambda n: [values[int(k)] for k in rng.integers(0, len(values), n)]) if values else (lambda n: [int.from_bytes(rng.bytes(16), "big") % F.p for _ in range(n)])
    cols = [draw(ln) for ln in lens]
    consts = draw(n_consts)
    return dom, cols, ([ln.bit_length() - 1 for ln in lens] if periodic else None), consts, stark.compile_transitions(build(stark))


def descriptors(F, n_transitions, seed, end_exemptions=1):
    coeffs = rand_elems(F, n_transitions, seed)
    return [dict(period=1, offset=0, end_exemptions=end_exemptions + c % 2, coeff=coeffs[c]) for c in range(n_transitions)]


# ---- the example AIRs
@pytest.mark.parametrize("shape", [(3, 2), (8, 2)], ids=["one_block", "several_blocks"])
@pytest.mark.parametrize("air", sorted(A.AIRS))
@pytest.mark.parametrize("field", FIELDS)
def test_example_airs(field, air, shape):
    F = M.FIELDS[field]
    dom, cols, lens, consts, program = air_inputs(F, air, shape[0], shape[1], 11)
    gammas = rand_elems(F, 2, 12)
    boundary = [(0, 0, 5, gammas[0]), (0, dom.n - 1, 7, gammas[1])]
    check(F, dom, cols, program, consts, boundary, descriptors(F, program.n_transitions, 13), lens=lens)


# ---- the zerofier, one branch at a time: one transition with coefficient 1, no boundary
ZEROFIERS = {
    "no_exemptions": dict(period=1, offset=0, end_exemptions=0),
    "one_exemption": dict(period=1, offset=0, end_exemptions=1),
    "two_exemptions": dict(period=1, offset=0, end_exemptions=2),
    "period_2_offset_1": dict(period=2, offset=1, end_exemptions=1),
    "exemptions_period": dict(period=2, offset=1, end_exemptions=1, exemptions_period=4, periodic_exemptions_offset=1),
    "odd_period": dict(period=3, offset=1, end_exemptions=2),   # the divisions truncate, the table is no power of two long
}


@pytest.mark.parametrize("branch", sorted(ZEROFIERS))
@pytest.mark.parametrize("field", FIELDS)
def test_zerofier_branches(field, branch):
    F = M.FIELDS[field]
    dom, cols, lens, consts, program = air_inputs(F, "quadratic", 4, 2, 21)
    check(F, dom, cols, program, consts, [], [dict(ZEROFIERS[branch], coeff=M.lift(F, 1))])


@pytest.mark.parametrize("field", FIELDS)
def test_identical_descriptors_share_a_class(field):
    F = M.FIELDS[field]
    dom, cols, lens, consts, program = air_inputs(F, "rom", 4, 2, 22)
    same, other = dict(period=2, offset=1, end_exemptions=1), dict(period=1, offset=0, end_exemptions=2)
    coeffs = rand_elems(F, 3, 23)
    check(F, dom, cols, program, consts, [], [dict(same, coeff=coeffs[0]), dict(other, coeff=coeffs[1]), dict(same, coeff=coeffs[2])])


def many_constraints(n):
    return stark.compile_transitions([stark.cell(0, 1 + k % 3) - stark.cell(0) for k in range(n)])


@pytest.mark.parametrize("field", FIELDS)
def test_descriptor_cap(field):
    F = M.FIELDS[field]
    dom = M.domain(F, 5, 2, 3)
    cols = [A.fill(F.p, dom.N, 24)]
    coeffs = rand_elems(F, R2_CLASSES + 1, 25)
    full = [dict(period=1, offset=0, end_exemptions=c, coeff=coeffs[c]) for c in range(R2_CLASSES)]
    check(F, dom, cols, many_constraints(R2_CLASSES), [], [], full)
    with pytest.raises(errors.HipError, match="distinct transition zerofiers"):
        device_call(F, dom, cols, many_constraints(R2_CLASSES + 1), [], [], full + [dict(period=1, offset=0, end_exemptions=R2_CLASSES, coeff=coeffs[-1])])


# ---- the boundary part
@pytest.mark.parametrize("field", FIELDS)
def test_boundary_steps(field):
    F = M.FIELDS[field]
    dom, cols, lens, consts, program = air_inputs(F, "fib2", 4, 2, 31)
    g = rand_elems(F, 8, 32)
    trs = descriptors(F, 2, 33)
    n = dom.n
    check(F, dom, cols, program, consts, [(0, 0, 1, g[0]), (1, n - 1, 2, g[1]), (1, 0, F.p - 1, g[2])], trs)        # two constraints on step 0
    many = [(k % 2, step, 3 + k, g[k]) for k, step in enumerate([5, 0, 9, 5, n - 1, 2, 7, n + 2])]                     # 6 distinct steps (n + 2 = 2 mod n)
    assert len({s % n for _, s, _, _ in many}) > R2_STEPS
    check(F, dom, cols, program, consts, many, trs)
    check(F, dom, cols, program_of([], 0), consts, many, [])            # n_transitions = 0: the program is empty too
    check(F, dom, cols, program, consts, [], trs)                       # n_boundary = 0


@pytest.mark.parametrize("field", FIELDS)
def test_no_transitions_and_nothing_at_all(field):
    F = M.FIELDS[field]
    dom = M.domain(F, 3, 2, 3)
    cols = [A.fill(F.p, dom.N, 34)]
    empty = program_of([], 0)
    check(F, dom, cols, empty, [], [(0, 1, 4, rand_elems(F, 1, 35)[0])], [])
    t_out = dev(field, [1] * (F.width * dom.N))
    assert device_call(F, dom, cols, empty, [], [], [], t_out=t_out) == [F.zero] * dom.N


# ---- operands at the edges
@pytest.mark.parametrize("air", ["rom", "fib_rap", "periodic"])
@pytest.mark.parametrize("field", FIELDS)
def test_edge_cells_constants_and_coefficients(field, air):
    F = M.FIELDS[field]
    dom, cols, lens, consts, program = air_inputs(F, air, 4, 2, 41, values=[0, 1, F.p - 1])
    top = (F.p - 1,) * F.width
    trs = [dict(period=1, offset=0, end_exemptions=1, coeff=top) for _ in range(program.n_transitions)]
    check(F, dom, cols, program, consts, [(0, 0, F.p - 1, top), (0, 3, 0, top)], trs, lens=lens)


def test_goldilocks_words_that_are_not_canonical():
    F = M.GL2
    dom, cols, lens, consts, program = air_inputs(F, "fib2", 4, 2, 42, values=[0, 1, F.p - 1])
    rng = np.random.default_rng(43)
    raw_values = [0, 1, F.p - 1, F.p, F.p + 1, (1 << 64) - 1]
    raw = [[raw_values[int(k)] for k in rng.integers(0, 6, dom.N)] for _ in cols]
    cols = [[F.unword(w) for w in c] for c in raw]
    check(F, dom, cols, program, consts, [(0, 0, 2, (F.p - 1, F.p - 1))], descriptors(F, 2, 44), raw_cols=raw)


@pytest.mark.parametrize("field", FIELDS)
def test_all_eight_temporaries(field):
    F = M.FIELDS[field]
    dom = M.domain(F, 5, 2, 3)
    cols = [A.fill(F.p, dom.N, 45 + c) for c in range(2)]
    program = stark.compile_transitions([A.all_temporaries(stark)])
    assert program.n_tmps == A.MAX_TMPS
    check(F, dom, cols, program, [], [(1, 2, 9, rand_elems(F, 1, 47)[0])], descriptors(F, 1, 48))


@pytest.mark.parametrize("field", FIELDS)
def test_program_of_the_maximal_length(field):
    F = M.FIELDS[field]
    dom = M.domain(F, 4, 1, 3)
    cols = [A.fill(F.p, dom.N, 49 + c) for c in range(2)]
    ops = [(A.LOAD, A.CELL, 0, 0)] + [((A.ADD, A.MUL, A.SUB)[k % 3], A.CELL, k % 2, k % dom.n) for k in range(A.MAX_OPS - 2)] + [(A.EMIT, 0, 0, 0)]
    assert len(ops) == A.MAX_OPS
    check(F, dom, cols, program_of(ops, 1), [], [], descriptors(F, 1, 51))


# ---- the output's stride
@pytest.mark.parametrize("field", FIELDS)
def test_out_stride_leaves_the_gap_untouched(field):
    F = M.FIELDS[field]
    dom, cols, lens, consts, program = air_inputs(F, "fib2", 4, 2, 61)
    stride, mark = dom.N + 8, 0x5A5A5A5A
    t_out = dev(field, [mark] * (F.width * stride))
    boundary, trs = [(0, 0, 1, rand_elems(F, 1, 62)[0])], descriptors(F, 2, 63)
    got = device_call(F, dom, cols, program, consts, boundary, trs, t_out=t_out, out_stride=stride)
    assert got == M.evaluate(F, dom, cols, program.ops.tolist(), consts, boundary, trs)
    words = host(field, t_out).reshape(F.width, stride)
    assert (words[:, dom.N:] == mark).all()


# ---- the parts
@pytest.mark.parametrize("n_parts", [1, 2, 3, 4])
@pytest.mark.parametrize("field", FIELDS)
def test_composition_parts(field, n_parts):
    F = M.FIELDS[field]
    dom = M.domain(F, 4, 2, 3)
    N, D = dom.N, F.width
    H = [A.fill(F.p, 41, 71 + e) + [0] * (N - 41) for e in range(D)]                # 41 coefficients: the lengths are not the blocks'
    evals = list(zip(*[M.R2.evaluate_on_coset(dom, h) for h in H]))
    t_evals = dev(field, [F.word(v[e]) for e in range(D) for v in evals])
    t_coeffs, lens, t_lde = MOD[field].composition_parts_device(t_evals, dom.log2_lde, n_parts, offset=F.word(dom.h))
    want_coeffs, want_lens, want_lde = M.parts(F, dom, evals, n_parts)
    L = MOD[field].part_block_len(dom.log2_lde, n_parts)
    got_coeffs = [[F.unword(w) for w in plane] for plane in host(field, t_coeffs).reshape(n_parts * D, L)]
    got_lde = [[F.unword(w) for w in plane] for plane in host(field, t_lde).reshape(n_parts * D, N)]
    assert got_coeffs == want_coeffs            # against the interpolation by definition
    assert got_lde == want_lde                  # against Horner on the coset
    assert lens == want_lens and lens == [len(range(j, 41, n_parts)) for j in range(n_parts)]
    # H(x_i) = sum_j x_i^j H_j(x_i^P) on the whole domain, from what the device wrote
    for i, x in enumerate(dom.coset):
        xp = pow(x, n_parts, F.p)
        for e in range(D):
            total = 0
            for j in range(n_parts):
                acc = 0
                for c in reversed(got_coeffs[j * D + e]):
                    acc = (acc * xp + c) % F.p
                total = (total + pow(x, j, F.p) * acc) % F.p
            assert total == evals[i][e]


# ---- the prover's own check, end to end, and the commitment
@functools.lru_cache(maxsize=None)
def fibonacci_round2(field, n_parts):
    """a satisfying Fibonacci trace of 2^6 rows, blow-up 4: LDE -> round2_device"""
    F = M.FIELDS[field]
    log2_trace, log2_blowup = 6, 2
    dom = M.domain(F, log2_trace, log2_blowup, 3)
    a, b = [1], [1]
    for _ in range(dom.n - 1):
        a, b = a + [b[-1]], b + [(a[-1] + b[-1]) % F.p]
    trace_dom = M.domain(F, log2_trace, 0, 1)
    polys = [M.interpolate(trace_dom, col) for col in (a, b)]
    t_polys = dev(field, [F.word(c) for poly in polys for c in poly])
    t_lde = torch.zeros(2 * dom.N, dtype=TORCH[field], device="cuda")
    if field == "gl2":
        goldilocks.lde_device(t_polys, log2_trace, t_lde, dom.log2_lde, batch=2, offset=dom.h)
    else:
        fft.lde_device(fft.Babybear31PrimeFieldU32, t_polys, log2_trace, t_lde, dom.log2_lde, batch=2, offset=np.array([F.word(dom.h)], np.uint32))
    coeffs = rand_elems(F, 4, 81)
    program = stark.compile_transitions(A.AIRS["fib2"][0](stark))
    transitions = [dict(period=1, offset=0, end_exemptions=1, coeff=coeffs[0]), dict(period=1, offset=0, end_exemptions=1, coeff=coeffs[1])]
    boundary = [(0, 0, 1, coeffs[2]), (1, 0, 1, coeffs[3])]
    bnd = [(col, step, F.word(value), F.word_elem(coeff)) for col, step, value, coeff in boundary]
    trs = [dict(t, coeff=F.word_elem(t["coeff"])) for t in transitions]
    out = MOD[field].round2_device(program, [], [t_lde[:dom.N], t_lde[dom.N:]], log2_trace, log2_blowup, bnd, trs, n_parts, offset=F.word(dom.h))
    return F, dom, polys, t_polys, program, boundary, transitions, out


@pytest.mark.parametrize("field", FIELDS)
def test_the_provers_check_at_an_out_of_domain_point(field):
    n_parts = 2
    F, dom, polys, t_polys, program, boundary, transitions, (t_coeffs, lens, t_lde, t_nodes, root) = fibonacci_round2(field, n_parts)
    E, D, X = F.ext, F.width, MOD[field]
    L = X.part_block_len(dom.log2_lde, n_parts)
    z = rand_elems(F, 1, 82)[0]
    zg = E.mul_base(z, dom.g)
    # the trace polynomials at z and z g, from the device
    trace_at = X.evaluate_device(t_polys, 2, dom.n, [F.word_elem(z), F.word_elem(zg)])
    for k in range(2):
        for j, pt in enumerate((z, zg)):
            assert F.unword_elem(trace_at[k, j]) == M.horner_ext(F, [M.lift(F, c) for c in polys[k]], pt)
    want = M.composition_at(F, dom, polys, program.ops.tolist(), [], boundary, transitions, z)
    # sum_j z^j H_j(z^P), the parts at z^P from the device
    zp, total = E.power(z, n_parts), F.zero
    for j in range(n_parts):
        hj = X.evaluate_ext_device(t_coeffs[j * D * L:(j + 1) * D * L], L, [F.word_elem(zp)])[0]
        total = E.add(total, E.mul(E.power(z, j), F.unword_elem(hj)))
    assert total == want
    # the trace satisfies the AIR: H has degree below n, every coefficient from n on is zero
    planes = host(field, t_coeffs).reshape(n_parts * D, L)
    for j in range(n_parts):
        first_zero = len(range(j, dom.n, n_parts))
        assert not planes[j * D:(j + 1) * D, first_zero:].any()
        assert lens[j] <= first_zero
    assert any(lens)


@pytest.mark.parametrize("field", FIELDS)
def test_the_commitment_is_the_column_commitment_of_the_planes(field):
    n_parts = 2
    F, dom, _, _, _, _, _, (t_coeffs, lens, t_lde, t_nodes, root) = fibonacci_round2(field, n_parts)
    t_again = torch.zeros_like(t_nodes)
    if field == "gl2":
        direct = rpo.commit_columns_device(goldilocks_ext.RPO_128, t_lde, n_parts * 2, dom.log2_lde, t_again)
        assert np.array_equal(np.asarray(root), np.asarray(direct))
    else:
        direct = merkle.commit_columns_layout_device(fft.Babybear31PrimeFieldU32, t_lde, n_parts * 4, dom.log2_lde, t_again)
        assert bytes(root) == bytes(direct)
    assert torch.equal(t_nodes, t_again)
