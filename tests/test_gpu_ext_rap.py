"""The randomized AIR over Goldilocks with Fp2 and over BabyBear with Fp4 on the device (csrc/ext_aux.cuh and the _rap_ part of
csrc/ext_round2.cuh) against the model of tests/ext_rap_ref.py, bit for bit: the auxiliary column as a running product or
sum of fractions, the constraint evaluations of a program that reads auxiliary columns and constants of the extension, the
prover's own check at an out-of-domain point and one chain from the main trace to a constant last FRI layer.

Launch boundaries (the constants of ext_aux.cuh): a work-item takes EXT_AUX_E = 4 rows and a workgroup a tile of 1024; the
carry kernel has EXT_AUX_TOP = 64 work-items, so 65 tiles give its first work-item two tiles and cross every level of the
scan.  The shapes are the smallest that reach each of them."""
import functools

import numpy as np
import pytest
import torch

from lambda_elliptic_curves_amd import babybear_ext, errors, fft, goldilocks, goldilocks_ext, stark
from tests import air_program_ref as A
from tests import ext_rap_ref as R
from tests import ext_round2_ref as M

pytestmark = pytest.mark.gpu
FIELDS = ["gl2", "bb4"]
TILE, TOP = 1024, 64
MOD = {"gl2": goldilocks_ext, "bb4": babybear_ext}
NP = {"gl2": np.uint64, "bb4": np.uint32}
TORCH = {"gl2": torch.int64, "bb4": torch.int32}
SIGNED = {"gl2": np.int64, "bb4": np.int32}
MODES = [(R.PRODUCT, False), (R.PRODUCT, True), (R.SUM, False), (R.SUM, True)]
MODE_IDS = ["product", "product_exclusive", "sum", "sum_exclusive"]


def dev(name, words):
    return torch.from_numpy(np.array(words, dtype=NP[name], order="C").view(SIGNED[name])).cuda()


def host(name, t):
    return t.cpu().numpy().view(NP[name])


def rand_words(F, n, seed):
    rng = np.random.default_rng(seed)
    return [int(x) % F.p for x in rng.integers(0, 1 << 62, n)]


def rand_elems(F, n, seed):
    rng = np.random.default_rng(seed)
    return [tuple(int.from_bytes(rng.bytes(16), "big") % F.p for _ in range(F.width)) for _ in range(n)]


def elems_of(F, t, n, stride=0):
    planes = host(F.name, t)
    stride = stride or n
    return [tuple(F.unword(planes[e * stride + i]) for e in range(F.width)) for i in range(n)]


# ---- the auxiliary column
def words_side(F, side):
    return (F.word_elem(side[0]), [(col, F.word_elem(coeff)) for col, coeff in side[1]])


@functools.lru_cache(maxsize=None)
def aux_case(field, n, shape):
    """-> (canonical columns, the words that go to the device, numerator, denominator, the fractions' model per mode)"""
    F = M.FIELDS[field]
    one = R.one(F)
    if shape == "four_terms":
        cols = [rand_words(F, n, 100 + k) for k in range(3)]
        c = rand_elems(F, 6, 110)
        num, den = (c[0], [(0, c[1]), (1, c[2])]), (c[3], [(2, c[4]), (0, c[5])])
    elif shape == "no_numerator":
        cols = [rand_words(F, n, 120)]
        c = rand_elems(F, 2, 121)
        num, den = (one, []), (c[0], [(0, c[1])])
    elif shape == "sixteen_terms":
        cols = [rand_words(F, n, 130 + k) for k in range(5)]
        c = rand_elems(F, 34, 135)
        num, den = (c[0], [(k % 5, c[1 + k]) for k in range(16)]), (c[17], [((3 * k + 1) % 5, c[18 + k]) for k in range(16)])
    elif shape == "same_column":
        cols = [rand_words(F, n, 140)]
        c = rand_elems(F, 4, 141)
        num, den = (c[0], [(0, c[1])]), (c[2], [(0, c[3])])
    else:   # "edges": the edge words in the columns and the coefficients; the constants are random, so that no denominator is zero
        values = [0, 1, F.p - 1]
        rng = np.random.default_rng(150)
        cols = [[values[int(k)] for k in rng.integers(0, 3, n)] for _ in range(3)]
        c = rand_elems(F, 2, 151)
        top, mixed = (F.p - 1,) * F.width, (0, 1, F.p - 1, 1)[:F.width]
        num, den = (c[0], [(0, top), (1, mixed), (2, one)]), (c[1], [(1, top), (2, mixed), (0, F.zero)])
    raw = [[F.word(v) for v in col] for col in cols]
    if shape == "edges" and field == "gl2":   # any u64 is a word: p, p + 1 and 2^64 - 1 stand for 0, 1 and 2^32 - 2
        above = {0: F.p, 1: F.p + 1}
        raw = [[above.get(v, v) if (i + k) % 2 else v for i, v in enumerate(col)] for k, col in enumerate(cols)]
        raw[0][n // 2], cols[0][n // 2] = (1 << 64) - 1, F.unword((1 << 64) - 1)
    values, zeros = R.fraction_values(F, cols, n, num, den)
    assert zeros == 0
    want = {m: R.running(F, values, *m) for m in MODES}
    return cols, raw, num, den, want


def check_aux(field, n, shape, mode, out_stride=0):
    F = M.FIELDS[field]
    cols, raw, num, den, want = aux_case(field, n, shape)
    t_cols = [dev(field, c) for c in raw]
    stride, mark = out_stride or n, 0x5A5A5A5A
    t_out = dev(field, [mark] * (F.width * stride))
    t_out, t_total = MOD[field].aux_fractions_device(t_cols, n, words_side(F, num), words_side(F, den), mode=mode[0], exclusive=mode[1], t_out=t_out,
                                                     out_stride=out_stride, total=True, count_zeros=True)
    column, total = want[mode]
    assert elems_of(F, t_out, n, stride) == column
    assert F.unword_elem(host(field, t_total)[:F.width]) == total
    inclusive = want[(mode[0], False)][0]
    assert total == inclusive[-1]                   # the total is the last inclusive value
    if out_stride:
        assert (host(field, t_out).reshape(F.width, stride)[:, n:] == mark).all()


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("n", [1, 2, TILE - 1, TILE, TILE + 1, 2 * TILE + 1])
@pytest.mark.parametrize("field", FIELDS)
def test_aux_lengths(field, n, mode):
    check_aux(field, n, "four_terms", mode)


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("field", FIELDS)
def test_aux_more_tiles_than_the_carry_kernel_has_work_items(field, mode):
    n = TOP * TILE + 1
    assert -(-n // TILE) == TOP + 1
    check_aux(field, n, "same_column", mode)


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("shape", ["no_numerator", "sixteen_terms", "same_column", "edges"])
@pytest.mark.parametrize("field", FIELDS)
def test_aux_list_shapes_and_edge_operands(field, shape, mode):
    check_aux(field, TILE + 5, shape, mode)


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("field", FIELDS)
def test_aux_out_stride_leaves_the_gap_untouched(field, mode):
    check_aux(field, TILE + 1, "four_terms", mode, out_stride=TILE + 1 + 8)


@pytest.mark.parametrize("mode", [MODES[0], MODES[3]], ids=[MODE_IDS[0], MODE_IDS[3]])
@pytest.mark.parametrize("field", FIELDS)
def test_aux_a_zero_denominator_in_the_last_tile(field, mode):
    F = M.FIELDS[field]
    n, b0 = 2 * TILE + 1, 12345
    col = rand_words(F, n, 160)
    col[2 * TILE] = F.p - b0                       # b0 + col = 0 in the only row of the last tile
    num, den = (R.one(F), []), (M.lift(F, b0), [(0, R.one(F))])
    assert R.aux_fractions(F, [col], n, num, den, *mode)[2] == 1
    t_col = dev(field, [F.word(v) for v in col])
    with pytest.raises(errors.FieldError, match=r"\[-10\].*1 rows have a zero denominator") as caught:
        MOD[field].aux_fractions_device([t_col], n, words_side(F, num), words_side(F, den), mode=mode[0], exclusive=mode[1], count_zeros=True)
    assert caught.value.zero_denominators == 1
    with pytest.raises(errors.FieldError, match=r"\[-10\]") as caught:   # round 1 reports it before anything is transformed
        short = col[:2 * TILE - 1] + [F.p - b0]        # a trace of 2^11 rows, the zero in its last row
        MOD[field].round1_aux_device([dev(field, [F.word(v) for v in short])], 11, 1, words_side(F, num), words_side(F, den), mode=mode[0],
                                     exclusive=mode[1], offset=F.word(3), count_zeros=True)
    assert caught.value.zero_denominators == 1
    MOD[field].aux_fractions_device([t_col], n, words_side(F, num), words_side(F, den), mode=mode[0], exclusive=mode[1])   # not asked for: only enqueued
    torch.cuda.synchronize()


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_aux_goldilocks_scalars_that_are_not_canonical(mode):
    """any u64 is a word of a host scalar too: p, p + 1 and 2^64 - 1 in the constants and the coefficients.  a_0 = (p + 1, p) is
    the one of Fp2, so a numerator without terms takes the path that skips its products"""
    F, n = M.GL2, TILE + 3
    p, top = F.p, (1 << 64) - 1
    cols = [rand_words(F, n, 165), rand_words(F, n, 166)]
    raw_num, raw_den = ((p + 1, p), []), ((top, p + 1), [(0, (p, top)), (1, (p + 1, p)), (0, (top, top))])
    canon = lambda side: (F.unword_elem(side[0]), [(col, F.unword_elem(c)) for col, c in side[1]])
    num, den = canon(raw_num), canon(raw_den)
    assert num == (R.one(F), []) and den[0] == (F.unword(top), 1)
    values, zeros = R.fraction_values(F, cols, n, num, den)
    assert zeros == 0
    want, total = R.running(F, values, *mode)
    t_out, t_total = goldilocks_ext.aux_fractions_device([dev("gl2", c) for c in cols], n, raw_num, raw_den, mode=mode[0], exclusive=mode[1], total=True,
                                                         count_zeros=True)
    assert elems_of(F, t_out, n) == want and F.unword_elem(host("gl2", t_total)[:2]) == total
    # the same numerator written canonically gives the same bytes
    t_again, _ = goldilocks_ext.aux_fractions_device([dev("gl2", c) for c in cols], n, ((1, 0), []), raw_den, mode=mode[0], exclusive=mode[1])
    assert torch.equal(t_out, t_again)


def test_rap_goldilocks_scalars_that_are_not_canonical():
    """p, p + 1 and 2^64 - 1 in the constants of E, the boundary values and the coefficients of the RAP entry"""
    F = M.GL2
    p, top = F.p, (1 << 64) - 1
    dom = M.domain(F, 3, 2, 3)
    cols = [rand_words(F, dom.N, 167 + k) for k in range(2)]
    aux = [rand_elems(F, dom.N, 169)]
    program = stark.compile_transitions(R.RAP_AIRS["fib_rap"][0](stark))
    raw_x, raw_beta = [(top, p + 1)], (p + 1, top)
    raw_bnd = [(0, 1, (top, p), (p, p + 1), True), (1, 2, (p + 1, top), (top, top), False), (0, 2, top, (p + 1, p), False)]
    t_cols = [dev("gl2", c) for c in cols]
    t_aux = [dev("gl2", [v[e] for e in range(2) for v in c]) for c in aux]
    t = goldilocks_ext.rap_constraint_evaluations_device(program, [], raw_x, t_cols, t_aux, 3, 2, raw_bnd, [dict(period=1, end_exemptions=1, coeff=raw_beta)],
                                                         offset=3)
    un = lambda v: F.unword_elem(v) if isinstance(v, tuple) else F.unword(v)
    want = R.evaluate(F, dom, cols, aux, program.ops.tolist(), [], [un(raw_x[0])], [(c, s, un(v), un(g), a) for c, s, v, g, a in raw_bnd],
                      [dict(period=1, end_exemptions=1, coeff=un(raw_beta))])
    assert elems_of(F, t, dom.N) == want


@pytest.mark.parametrize("field", FIELDS)
def test_aux_columns_of_the_two_examples(field):
    """read_only_memory.rs (inclusive) and fibonacci_rap.rs (exclusive) with challenges whose coordinates are all non-zero,
    against the two loops of the reference restated in ext_rap_ref"""
    F, E, X = M.FIELDS[field], M.FIELDS[field].ext, MOD[field]
    one, n = R.one(F), 64
    z, alpha, gamma = rand_elems(F, 3, 170)
    assert all(all(c) for c in (z, alpha, gamma))
    # a read-only memory of n / 2 cells, each read twice, and the same reads sorted by address
    rng = np.random.default_rng(171)
    values = rand_words(F, n // 2, 172)
    a = [int(x) for x in rng.permutation(np.repeat(np.arange(n // 2), 2))]
    v = [values[x] for x in a]
    a_sorted = sorted(a)
    v_sorted = [values[x] for x in a_sorted]
    t_cols = [dev(field, [F.word(x) for x in c]) for c in (a, v, a_sorted, v_sorted)]
    neg = lambda e: E.sub(F.zero, e)
    t_out, t_total = X.aux_fractions_device(t_cols, n, (F.word_elem(z), [(0, F.word_elem(neg(one))), (1, F.word_elem(neg(alpha)))]),
                                            (F.word_elem(z), [(2, F.word_elem(neg(one))), (3, F.word_elem(neg(alpha)))]), total=True, count_zeros=True)
    want = R.rom_aux_column(F, a, v, a_sorted, v_sorted, z, alpha)
    assert elems_of(F, t_out, n) == want and want[-1] == one
    assert F.unword_elem(host(field, t_total)[:F.width]) == one
    # fibonacci_rap_trace([1, 1], 31): the sequence, its copy with the ends swapped, a row of zeros
    fib = [1, 1]
    while len(fib) < 31:
        fib.append((fib[-1] + fib[-2]) % F.p)
    perm = [fib[-1]] + fib[1:-1] + [fib[0]]
    fib, perm = fib + [0], perm + [0]
    t_cols = [dev(field, [F.word(x) for x in c]) for c in (fib, perm)]
    t_out, _ = X.aux_fractions_device(t_cols, 32, (F.word_elem(gamma), [(0, F.word_elem(one))]), (F.word_elem(gamma), [(1, F.word_elem(one))]),
                                      exclusive=True, count_zeros=True)
    want = R.fib_rap_aux_column(F, fib, perm, gamma)
    assert elems_of(F, t_out, 32) == want and want[-1] == one


# ---- round 2 with auxiliary columns and constants of the extension
SHAPES = [(3, 2), (8, 2)]          # N = 32 and N = 1024
SHAPE_IDS = ["N32", "N1024"]


def program_of(ops, n_transitions):
    return stark.AirProgram(np.array(ops, dtype=stark.AIR_OP_DTYPE), n_transitions)


def rap_call(F, dom, cols, aux, program, consts, xconsts, boundary, transitions, t_out=None, out_stride=0):
    """canonical inputs -> the N elements of E, canonical, from the RAP entry"""
    name, log2_trace = F.name, dom.n.bit_length() - 1
    t_cols = [dev(name, [F.word(v) for v in c]) for c in cols]
    t_aux = [dev(name, [F.word(v[e]) for e in range(F.width) for v in c]) for c in aux]
    bnd = [(col, step, F.word_elem(value) if isinstance(value, tuple) else F.word(value), F.word_elem(coeff), is_aux) for col, step, value, coeff, is_aux in boundary]
    trs = [dict(t, coeff=F.word_elem(t["coeff"])) for t in transitions]
    t = MOD[name].rap_constraint_evaluations_device(program, [F.word(c) for c in consts], [F.word_elem(c) for c in xconsts], t_cols, t_aux, log2_trace,
                                                    dom.log2_lde - log2_trace, bnd, trs, t_out=t_out, out_stride=out_stride, offset=F.word(dom.h))
    return elems_of(F, t, dom.N, out_stride)


def check_rap(F, dom, cols, aux, program, consts, xconsts, boundary, transitions):
    got = rap_call(F, dom, cols, aux, program, consts, xconsts, boundary, transitions)
    want = R.evaluate(F, dom, cols, aux, program.ops.tolist(), consts, xconsts, boundary, transitions)
    assert got == want


def descriptors(F, n_transitions, seed, end_exemptions=1):
    coeffs = rand_elems(F, n_transitions, seed)
    return [dict(period=1, offset=0, end_exemptions=end_exemptions + c % 2, coeff=coeffs[c]) for c in range(n_transitions)]


def rap_inputs(F, shape, n_cols, n_aux, seed):
    dom = M.domain(F, shape[0], shape[1], 3)
    cols = [rand_words(F, dom.N, seed + k) for k in range(n_cols)]
    aux = [rand_elems(F, dom.N, seed + 50 + k) for k in range(n_aux)]
    return dom, cols, aux


@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
@pytest.mark.parametrize("field", FIELDS)
def test_a_program_without_the_new_sources_gives_the_existing_entrys_output(field, shape):
    F, X = M.FIELDS[field], MOD[field]
    dom, cols, _ = rap_inputs(F, shape, 5, 0, 200)
    program = stark.compile_transitions(A.AIRS["rom"][0](stark))
    consts = [F.word(c) for c in rand_words(F, 3, 201)]
    g = rand_elems(F, 3, 202)
    boundary = [(0, 0, F.word(5), F.word_elem(g[0])), (4, dom.n - 1, F.word(7), F.word_elem(g[1])), (2, 0, F.word(F.p - 1), F.word_elem(g[2]))]
    trs = [dict(t, coeff=F.word_elem(t["coeff"])) for t in descriptors(F, 3, 203)]
    t_cols = [dev(field, [F.word(v) for v in c]) for c in cols]
    log2_trace, log2_blowup = shape
    old = X.constraint_evaluations_device(program, consts, t_cols, log2_trace, log2_blowup, boundary, trs, offset=F.word(dom.h))
    new = X.rap_constraint_evaluations_device(program, consts, [], t_cols, [], log2_trace, log2_blowup, boundary, trs, offset=F.word(dom.h))
    assert torch.equal(old, new)
    assert host(field, new).any()


@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
@pytest.mark.parametrize("air", sorted(R.RAP_AIRS))
@pytest.mark.parametrize("field", FIELDS)
def test_the_two_examples_with_the_challenges_in_the_extension(field, air, shape):
    F = M.FIELDS[field]
    build, n_cols, n_consts, n_xconsts = R.RAP_AIRS[air]
    dom, cols, aux = rap_inputs(F, shape, n_cols, 1, 210)
    program = stark.compile_transitions(build(stark))
    g = rand_elems(F, 3, 211)
    boundary = [(0, 0, 5, g[0], False), (0, 0, g[2], g[1], True)]
    check_rap(F, dom, cols, aux, program, [1] * n_consts, rand_elems(F, n_xconsts, 212), boundary, descriptors(F, program.n_transitions, 213))


def every_pair(S):
    """ADD, SUB and MUL on F.F, F.E, E.F and E.E, NEG of both types; every one is emitted, so EMIT of both types as well"""
    out = []
    for k, op in enumerate(("add", "sub", "mul")):
        f, e = S.cell(0, k), S.xcell(0, k)
        ff, fe, ef, ee = f._bin(op, S.cell(1)), f._bin(op, S.xconst(0)), e._bin(op, S.const(0)), e._bin(op, S.xcell(1, 1))
        out += [ff, fe, ef, ee, -ff, -ee]
    return out


@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
@pytest.mark.parametrize("field", FIELDS)
def test_every_pair_of_operand_types(field, shape):
    F = M.FIELDS[field]
    dom, cols, aux = rap_inputs(F, shape, 2, 2, 220)
    program = stark.compile_transitions(every_pair(stark))
    words = R.type_program([tuple(o) for o in program.ops.tolist()], F.width)[0]
    seen = {(w & 7, (w >> 4) & 3) for w in words}
    assert {(op, t) for op in (A.ADD, A.SUB, A.MUL) for t in range(4)} <= seen and {(A.NEG, 0), (A.NEG, 1), (A.EMIT, 0), (A.EMIT, 1)} <= seen
    check_rap(F, dom, cols, aux, program, rand_words(F, 1, 221), rand_elems(F, 1, 222), [], descriptors(F, program.n_transitions, 223))


@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
@pytest.mark.parametrize("field", FIELDS)
def test_edge_operands_in_the_extension(field, shape):
    F = M.FIELDS[field]
    dom = M.domain(F, shape[0], shape[1], 3)
    values = [0, 1, F.p - 1]
    rng = np.random.default_rng(230)
    cols = [[values[int(k)] for k in rng.integers(0, 3, dom.N)] for _ in range(2)]
    aux = [[tuple(values[int(k)] for k in rng.integers(0, 3, F.width)) for _ in range(dom.N)] for _ in range(2)]
    top = (F.p - 1,) * F.width
    program = stark.compile_transitions(every_pair(stark))
    trs = [dict(period=1, offset=0, end_exemptions=1, coeff=top) for _ in range(program.n_transitions)]
    check_rap(F, dom, cols, aux, program, [F.p - 1], [top], [(0, 0, top, top, True), (1, 3, top, top, False)], trs)


@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
@pytest.mark.parametrize("field", FIELDS)
def test_eight_temporaries_all_in_the_extension(field, shape):
    F = M.FIELDS[field]
    dom, cols, aux = rap_inputs(F, shape, 2, 1, 240)
    e = stark.xcell(0, 0)
    for k in reversed(range(A.MAX_TMPS)):
        e = e * (stark.xcell(0, k % dom.n) + stark.cell(1, k % dom.n))
    program = stark.compile_transitions([e, stark.cell(0, 1) * stark.cell(1)])       # and one constraint in F after them
    assert R.type_program([tuple(o) for o in program.ops.tolist()], F.width)[1:] == (A.MAX_TMPS, A.MAX_TMPS, A.MAX_TMPS * F.width)
    trs = [dict(period=1, offset=0, end_exemptions=c, coeff=x) for c, x in enumerate(rand_elems(F, 2, 241))]   # two classes on top of the LDS maximum
    check_rap(F, dom, cols, aux, program, [], [], [], trs)


@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
@pytest.mark.parametrize("field", FIELDS)
def test_a_temporary_stored_as_a_word_and_overwritten_as_an_element(field, shape):
    F = M.FIELDS[field]
    dom, cols, aux = rap_inputs(F, shape, 2, 1, 250)
    ops = [(A.LOAD, A.CELL, 0, 0), (A.STORE, 0, 1, 0),                                            # tmp 1 = a word
           (A.LOAD, A.CELL, 1, 1), (A.MUL, A.TMP, 1, 0), (A.STORE, 0, 3, 0), (A.EMIT, 0, 0, 0),   # read as a word; tmp 3 = a word
           (A.LOAD, A.TMP, 1, 0), (A.MUL, R.XCONST, 0, 0), (A.STORE, 0, 1, 0),                     # tmp 1 = an element, over the word
           (A.LOAD, R.XCELL, 0, 1), (A.STORE, 0, 0, 0),                                           # tmp 0 = an element
           (A.LOAD, A.TMP, 3, 0), (A.SUB, A.TMP, 1, 0), (A.ADD, A.TMP, 0, 0), (A.STORE, 0, 3, 0), (A.EMIT, 0, 1, 0),   # F - E + E; tmp 3 = an element
           (A.LOAD, A.TMP, 3, 0), (A.NEG, 0, 0, 0), (A.MUL, A.TMP, 1, 0), (A.EMIT, 0, 2, 0)]
    assert R.type_program(ops, F.width)[1:] == (4, 3, 1 + 3 * F.width)
    check_rap(F, dom, cols, aux, program_of(ops, 3), [], rand_elems(F, 1, 251), [], descriptors(F, 3, 252))


@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
@pytest.mark.parametrize("field", FIELDS)
def test_an_auxiliary_cell_at_a_row_offset_that_wraps_the_domain(field, shape):
    F = M.FIELDS[field]
    dom, cols, aux = rap_inputs(F, shape, 1, 1, 260)
    program = stark.compile_transitions([stark.xcell(0, dom.n - 1) - stark.xcell(0) * stark.cell(0, dom.n - 1), stark.xcell(0, 1) + stark.xcell(0, dom.n // 2)])
    check_rap(F, dom, cols, aux, program, [], [], [], descriptors(F, 2, 261))


@pytest.mark.parametrize("n_steps", [1, 4, 5])
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
@pytest.mark.parametrize("field", FIELDS)
def test_boundary_constraints_on_auxiliary_and_main_columns(field, shape, n_steps):
    F = M.FIELDS[field]
    dom, cols, aux = rap_inputs(F, shape, 2, 2, 270)
    program = stark.compile_transitions(R.RAP_AIRS["fib_rap"][0](stark))
    trs = descriptors(F, 1, 271)
    n = dom.n
    steps = [0, n - 1, 5, n + 2, 3][:n_steps]            # n + 2 = 2 mod n
    g, v = rand_elems(F, 3 * n_steps, 272), rand_elems(F, 2 * n_steps, 273)
    on_aux = [(k % 2, s, v[k], g[k], True) for k, s in enumerate(steps)]
    on_main = [(k % 2, s, v[n_steps + k], g[n_steps + k], False) for k, s in enumerate(steps)]      # values with non-zero high coordinates
    assert all(all(c) for x in v for c in [x])
    check_rap(F, dom, cols, aux, program, [], rand_elems(F, 1, 274), on_aux, trs)
    check_rap(F, dom, cols, aux, program, [], rand_elems(F, 1, 274), on_main, trs)
    both = on_aux + on_main + [(0, s, 9 + k, g[2 * n_steps + k], False) for k, s in enumerate(steps)]   # both kinds at every step, a value in F too
    check_rap(F, dom, cols, aux, program, [], rand_elems(F, 1, 274), both, trs)
    check_rap(F, dom, cols, aux, program_of([], 0), [], [], both, [])                                  # no transitions: the boundary part alone


@pytest.mark.parametrize("field", FIELDS)
def test_rap_out_stride_leaves_the_gap_untouched(field):
    F = M.FIELDS[field]
    dom, cols, aux = rap_inputs(F, SHAPES[0], 2, 1, 280)
    program = stark.compile_transitions(R.RAP_AIRS["fib_rap"][0](stark))
    stride, mark = dom.N + 8, 0x5A5A5A5A
    t_out = dev(field, [mark] * (F.width * stride))
    xc, trs, bnd = rand_elems(F, 1, 281), descriptors(F, 1, 282), [(0, 1, rand_elems(F, 1, 283)[0], rand_elems(F, 1, 284)[0], True)]
    got = rap_call(F, dom, cols, aux, program, [], xc, bnd, trs, t_out=t_out, out_stride=stride)
    assert got == R.evaluate(F, dom, cols, aux, program.ops.tolist(), [], xc, bnd, trs)
    assert (host(field, t_out).reshape(F.width, stride)[:, dom.N:] == mark).all()


# ---- the prover's own check and one chain down to the last FRI layer
def extend(field, t_values, log2_trace, dom, batch):
    """`batch` dense planes of n values on the trace domain -> (their coefficients, their LDE on the coset)"""
    F = M.FIELDS[field]
    t_polys = torch.empty_like(t_values)
    t_lde = torch.zeros(batch * dom.N, dtype=TORCH[field], device="cuda")
    if field == "gl2":
        goldilocks.ntt_device(t_values, t_polys, log2_trace, inverse=True, batch=batch)
        goldilocks.lde_device(t_polys, log2_trace, t_lde, dom.log2_lde, batch=batch, offset=dom.h)
    else:
        fld = fft.Babybear31PrimeFieldU32
        fft.ntt_device(fld, t_values, t_polys, log2_trace, inverse=True, batch=batch)
        fft.lde_device(fld, t_polys, log2_trace, t_lde, dom.log2_lde, batch=batch, offset=np.array([F.word(dom.h)], np.uint32))
    return t_polys, t_lde


def fib_rap_air(F, dom, seed):
    """fibonacci_rap.rs with z as an auxiliary column: the program, the transitions and the boundary constraints"""
    S = stark
    gamma = S.xconst(0)
    program = S.compile_transitions([S.cell(0, 2) - S.cell(0, 1) - S.cell(0), S.xcell(0, 1) * (gamma + S.cell(1)) - S.xcell(0) * (gamma + S.cell(0))])
    c = rand_elems(F, 6, seed)
    transitions = [dict(period=1, offset=0, end_exemptions=3, coeff=c[0]), dict(period=1, offset=0, end_exemptions=1, coeff=c[1])]
    one = R.one(F)
    boundary = [(0, 0, 1, c[2], False), (0, 1, 1, c[3], False), (0, 0, one, c[4], True), (0, dom.n - 1, one, c[5], True)]
    return program, transitions, boundary


@functools.lru_cache(maxsize=None)
def fib_rap_round2(field, corrupt):
    """a satisfying fibonacci_rap trace of 2^5 rows, blow-up 4: main LDE, the auxiliary column from the device (one value
    changed before its LDE with `corrupt`), round2_rap_device"""
    F, X = M.FIELDS[field], MOD[field]
    log2_trace, log2_blowup, n_parts = 5, 2, 2
    dom = M.domain(F, log2_trace, log2_blowup, 3)
    n = dom.n
    fib = [1, 1]
    while len(fib) < n - 1:
        fib.append((fib[-1] + fib[-2]) % F.p)
    perm = [fib[-1]] + fib[1:-1] + [fib[0]]
    main = [fib + [0], perm + [0]]
    gamma = rand_elems(F, 1, 300)[0]
    trace_dom = M.domain(F, log2_trace, 0, 1)
    t_main = dev(field, [F.word(v) for col in main for v in col])
    t_main_polys, t_main_lde = extend(field, t_main, log2_trace, dom, 2)
    t_cols = [t_main[:n], t_main[n:]]
    num, den = (F.word_elem(gamma), [(0, F.word_elem(R.one(F)))]), (F.word_elem(gamma), [(1, F.word_elem(R.one(F)))])
    if corrupt:
        t_aux, t_total = X.aux_fractions_device(t_cols, n, num, den, exclusive=True, total=True)
        t_aux[n + 7] ^= 1                                            # one coordinate of one value
        t_aux_polys, t_aux_lde = extend(field, t_aux, log2_trace, dom, F.width)
        aux_nodes = aux_root = None
    else:
        t_aux, t_total, t_aux_polys, t_aux_lde, aux_nodes, aux_root = X.round1_aux_device(t_cols, log2_trace, log2_blowup, num, den, exclusive=True,
                                                                                           offset=F.word(dom.h))
    program, transitions, boundary = fib_rap_air(F, dom, 301)
    bnd = [(col, step, F.word_elem(value) if isinstance(value, tuple) else F.word(value), F.word_elem(coeff), is_aux) for col, step, value, coeff, is_aux in boundary]
    trs = [dict(t, coeff=F.word_elem(t["coeff"])) for t in transitions]
    out = X.round2_rap_device(program, [], [F.word_elem(gamma)], [t_main_lde[:dom.N], t_main_lde[dom.N:]], [t_aux_lde], log2_trace, log2_blowup, bnd, trs, n_parts,
                              offset=F.word(dom.h))
    polys = [M.interpolate(trace_dom, col) for col in main]
    return dict(F=F, dom=dom, main=main, gamma=gamma, polys=polys, t_main_polys=t_main_polys, t_main_lde=t_main_lde, t_aux=t_aux, t_total=t_total,
                t_aux_polys=t_aux_polys, t_aux_lde=t_aux_lde, aux_nodes=aux_nodes, aux_root=aux_root, program=program, transitions=transitions,
                boundary=boundary, out=out, n_parts=n_parts, trace_dom=trace_dom)


@pytest.mark.parametrize("field", FIELDS)
def test_the_provers_check_with_an_auxiliary_column(field):
    c = fib_rap_round2(field, False)
    F, dom, n_parts = c["F"], c["dom"], c["n_parts"]
    E, D, X, n = F.ext, F.width, MOD[field], dom.n
    t_coeffs, lens, t_lde, t_nodes, root = c["out"]
    # the column the device built is the reference's loop, the total its last inclusive value, the LDE that of its planes
    aux = R.fib_rap_aux_column(F, c["main"][0], c["main"][1], c["gamma"])
    assert elems_of(F, c["t_aux"], n) == aux and aux[-1] == R.one(F)
    assert F.unword_elem(host(field, c["t_total"])[:D]) == R.one(F)
    aux_planes = [M.interpolate(c["trace_dom"], [v[e] for v in aux]) for e in range(D)]
    aux_poly = list(zip(*aux_planes))
    assert [F.unword(w) for w in host(field, c["t_aux_polys"])] == [x for plane in aux_planes for x in plane]
    assert elems_of(F, c["t_aux_lde"], dom.N) == [M.horner_ext(F, aux_poly, M.lift(F, x)) for x in dom.coset]
    # H(z) from the parts against the constraints at z, aux(z) recombined from its planes
    z = rand_elems(F, 1, 302)[0]
    zg = E.mul_base(z, dom.g)
    aux_at = X.evaluate_ext_device(c["t_aux_polys"], n, [F.word_elem(z), F.word_elem(zg)])
    assert [F.unword_elem(v) for v in aux_at] == [M.horner_ext(F, aux_poly, pt) for pt in (z, zg)]
    want = R.composition_at(F, dom, c["polys"], [aux_poly], c["program"].ops.tolist(), [], [c["gamma"]], c["boundary"], c["transitions"], z)
    L = X.part_block_len(dom.log2_lde, n_parts)
    zp, total = E.power(z, n_parts), F.zero
    for j in range(n_parts):
        hj = X.evaluate_ext_device(t_coeffs[j * D * L:(j + 1) * D * L], L, [F.word_elem(zp)])[0]
        total = E.add(total, E.mul(E.power(z, j), F.unword_elem(hj)))
    assert total == want
    # the trace satisfies the AIR: H has degree below n
    planes = host(field, t_coeffs).reshape(n_parts * D, L)
    for j in range(n_parts):
        first_zero = len(range(j, n, n_parts))
        assert not planes[j * D:(j + 1) * D, first_zero:].any()
        assert lens[j] <= first_zero
    assert any(lens)


@pytest.mark.parametrize("field", FIELDS)
def test_a_corrupted_auxiliary_value_breaks_the_degree_bound(field):
    c = fib_rap_round2(field, True)
    _, lens, _, _, _ = c["out"]
    assert max(lens) > len(range(0, c["dom"].n, c["n_parts"]))


@pytest.mark.parametrize("field", FIELDS)
def test_one_chain_to_a_constant_last_fri_layer(field):
    c = fib_rap_round2(field, False)
    F, dom, n_parts = c["F"], c["dom"], c["n_parts"]
    E, D, X, n, N = F.ext, F.width, MOD[field], dom.n, dom.N
    t_coeffs, lens, t_parts_lde, t_nodes, root = c["out"]
    assert c["aux_root"] is not None and len(np.asarray(c["aux_root"]).tobytes()) >= 32 and np.asarray(c["aux_root"]).any()
    # OOD: the main columns and the planes of the auxiliary column at z and z g
    z = rand_elems(F, 1, 310)[0]
    pts = [F.word_elem(z), F.word_elem(E.mul_base(z, dom.g))]
    t_polys = torch.cat([c["t_main_polys"], c["t_aux_polys"]])
    n_cols = 2 + D
    evals = X.evaluate_device(t_polys, n_cols, n, pts)
    # DEEP over the main columns and the auxiliary planes, as 2 + D base columns
    weights = [[F.word_elem(w) for w in rand_elems(F, 2, 311 + k)] for k in range(n_cols)]
    t_cols = torch.cat([c["t_main_lde"], c["t_aux_lde"]])
    t_deep = torch.zeros(D * N, dtype=TORCH[field], device="cuda")
    X.deep_quotients_device(t_cols, n_cols, dom.log2_lde, pts, weights, [[tuple(int(x) for x in evals[k, j]) for j in range(2)] for k in range(n_cols)], t_deep,
                            offset=F.word(dom.h))
    # its coefficients: degree below n, since the evaluations are the columns' own
    t_deep_coeffs = torch.empty_like(t_deep)
    if field == "gl2":
        goldilocks.ntt_device(t_deep, t_deep_coeffs, dom.log2_lde, inverse=True, batch=D, offset=dom.h)
    else:
        fft.ntt_device(fft.Babybear31PrimeFieldU32, t_deep, t_deep_coeffs, dom.log2_lde, inverse=True, batch=D, offset=np.array([F.word(dom.h)], np.uint32))
    planes = host(field, t_deep_coeffs).reshape(D, N)
    assert not planes[:, n:].any() and planes[:, :n].any()
    t_low = t_deep_coeffs.reshape(D, N)[:, :n].contiguous().reshape(-1)
    zetas = rand_elems(F, dom.log2_lde, 320)
    feed = list(zetas)
    last, layers = X.fri_commit_phase_device(t_low, n, n.bit_length() - 1, F.word(dom.h), N, lambda prev: F.word_elem(feed.pop(0)))
    poly = [tuple(F.unword(planes[e, i]) for e in range(D)) for i in range(n)]
    for zeta in zetas[:n.bit_length() - 1]:
        poly = E.fold(poly, zeta)
    assert len(layers) == n.bit_length() - 2
    assert all(v == F.zero for v in poly[1:]) and F.unword_elem(last) == poly[0] and poly[0] != F.zero
