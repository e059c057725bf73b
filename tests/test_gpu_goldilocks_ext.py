"""The Goldilocks quadratic extension on the device (csrc/goldilocks_ext.cuh, goldilocks_ext.hip) against the model of
tests/goldilocks_ext_ref.py, bit for bit: the pointwise seam at the operand edges, out-of-domain evaluation, the DEEP
quotients, one FRI layer and the whole commit phase.

Launch boundaries (the constants of goldilocks_ext.hip): evaluate gives a work-item GE_E = 8 coefficients and a block
GE_TILE = 2048; the fold kernel gives a work-item one tile sum up to 256 tiles and two from 2^19 + 1 coefficients on; a
launch holds GE_PTS = 4 points.  DEEP gives a work-item GD_ROWS = 4 rows and a launch GD_PTS = 4 points.  The layer's
tree switches from the top kernel alone to pair launches above 2^9 leaves (TOP_LOG2), that is between the domains 2^10
and 2^11."""
import numpy as np
import pytest
import torch

from lambda_elliptic_curves_amd import fft, goldilocks, merkle
from lambda_elliptic_curves_amd import goldilocks_ext as E
from tests import goldilocks_ext_ref as X
from tests import goldilocks_ref as G
from tests import rpo_ref as R

pytestmark = pytest.mark.gpu
P = G.P
GE_E, GE_TILE, GE_PTS, GD_ROWS, GD_PTS = 8, 2048, 4, 4, 4
EDGE = np.array(G.EDGE, np.uint64)
LEVELS = [E.RPO_128, E.RPO_160]


def dev(a):
    return torch.from_numpy(np.array(a, dtype=np.uint64, order="C").view(np.int64)).cuda()


def host(t):
    return t.cpu().numpy().view(np.uint64)


def empty(n):
    return torch.zeros(n, dtype=torch.int64, device="cuda")


def rand_words(shape, seed):
    return np.random.default_rng(seed).integers(0, 1 << 64, shape, dtype=np.uint64)   # any u64: non-canonical words included


def rand_elems(n, seed):
    return [tuple(int(v) % P for v in row) for row in rand_words((n, 2), seed)]


def planes_of(elems):
    return np.array([[e[0] for e in elems], [e[1] for e in elems]], np.uint64)


def elems_of(planes):
    return [(int(a), int(b)) for a, b in zip(planes[0], planes[1])]


def edge_point(k):
    return (G.EDGE[(5 * k + 3) % 28], G.EDGE[(7 * k + 1) % 28 or 1])   # components from EDGE, c1 != 0


# ---- pointwise
def test_pointwise_mul_on_the_edge_operands():
    g = np.meshgrid(EDGE, EDGE, EDGE, EDGE, indexing="ij")
    a0, a1, b0, b1 = (x.reshape(-1) for x in g)
    n = a0.size
    assert n == 28 ** 4
    t_a, t_b, t_out = dev(np.stack([a0, a1])), dev(np.stack([b0, b1])), empty(2 * n)
    E.pointwise_device(E.MUL, t_a, t_b, t_out, n)
    want = X.np_mul(a0, a1, b0, b1)
    got = host(t_out).reshape(2, n)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert got[:, 1234].tolist() == list(X.mul((int(a0[1234]), int(a1[1234])), (int(b0[1234]), int(b1[1234]))))


def test_pointwise_sqr_inv_and_mul_base():
    g = np.meshgrid(EDGE, EDGE, indexing="ij")
    extra = rand_words((2, 1 << 12), 41)
    extra[0, 0], extra[1, 0], extra[0, 1], extra[1, 1], extra[:, 2] = P, (1 << 64) - 1, (1 << 64) - 1, P, 0
    a = np.concatenate([np.stack([x.reshape(-1) for x in g]), extra], axis=1)
    n = a.shape[1]
    elems = [X.elem(e) for e in elems_of(a)]
    t_a, t_out = dev(a), empty(2 * n)
    E.pointwise_device(E.SQR, t_a, None, t_out, n)
    assert elems_of(host(t_out).reshape(2, n)) == [X.sqr(e) for e in elems]
    E.pointwise_device(E.INV, t_a, None, t_out, n)
    inv = elems_of(host(t_out).reshape(2, n))
    assert inv == [X.inv(e) for e in elems]
    assert inv[0] == (0, 0) and inv[28 ** 2 + 2] == (0, 0)        # the inverse of zero is written as zero
    assert all(X.mul(e, v) == (1, 0) for e, v in zip(elems, inv) if e != (0, 0))
    # a b with b in F: EDGE^3
    g = np.meshgrid(EDGE, EDGE, EDGE, indexing="ij")
    a0, a1, b = (x.reshape(-1) for x in g)
    t_out = empty(2 * b.size)
    E.pointwise_device(E.MUL_BASE, dev(np.stack([a0, a1])), dev(b), t_out, b.size)
    want = X.np_mul_base(a0, a1, b)
    got = host(t_out).reshape(2, b.size)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


def test_pointwise_strides_in_place_and_one_element():
    n, sa, sb, so = 1000, 1003, 1024, 1501
    a, b = rand_words(sa + n, 42), rand_words(sb + n, 43)
    ae = [X.elem(e) for e in zip(a[:n].tolist(), a[sa:sa + n].tolist())]
    be = [X.elem(e) for e in zip(b[:n].tolist(), b[sb:sb + n].tolist())]
    fill = np.full(so + n, 0x5555, np.uint64)
    t_out = dev(fill)
    E.pointwise_device(E.MUL, dev(a), dev(b), t_out, n, sa, sb, so)
    got = host(t_out)
    assert list(zip(got[:n].tolist(), got[so:so + n].tolist())) == [X.mul(x, y) for x, y in zip(ae, be)]
    assert (got[n:so] == 0x5555).all()                            # the words between the planes are not touched
    # in place, over a and over b
    t_a, t_b = dev(a), dev(b)
    E.pointwise_device(E.MUL, t_a, t_b, t_a, n, sa, sb, sa)
    got = host(t_a)
    assert list(zip(got[:n].tolist(), got[sa:sa + n].tolist())) == [X.mul(x, y) for x, y in zip(ae, be)]
    assert np.array_equal(got[n:sa], a[n:sa])
    t_a = dev(a)
    E.pointwise_device(E.MUL, t_a, t_b, t_b, n, sa, sb, sb)
    got = host(t_b)
    assert list(zip(got[:n].tolist(), got[sb:sb + n].tolist())) == [X.mul(x, y) for x, y in zip(ae, be)]
    t_a = dev(a)
    E.pointwise_device(E.INV, t_a, None, t_a, n, sa, 0, sa)
    got = host(t_a)
    assert list(zip(got[:n].tolist(), got[sa:sa + n].tolist())) == [X.inv(x) for x in ae]
    # one element
    for op, f in ((E.MUL, X.mul), (E.SQR, lambda x, _: X.sqr(x)), (E.INV, lambda x, _: X.inv(x)), (E.MUL_BASE, lambda x, y: X.mul_base(x, y[0]))):
        t_out = empty(2)
        E.pointwise_device(op, dev([P - 2, 1 << 63]), dev([P - 1, 3]), t_out, 1)
        assert tuple(host(t_out).tolist()) == f((P - 2, 1 << 63), (P - 1, 3))


# ---- evaluate
_EVAL = {}


def eval_case(n):
    """3 columns of n coefficients, 16 words of other data between two columns; shared by the cases of one length"""
    if n not in _EVAL:
        stride = n + 16
        words = rand_words(3 * stride, 50 + n % 97)
        words[0], words[min(1, n - 1)] = P, (1 << 64) - 1
        _EVAL[n] = (stride, words, dev(words))
    return _EVAL[n]


@pytest.mark.parametrize("n", [1, 2, 3, GE_E - 1, GE_E, GE_E + 1, GE_TILE - 1, GE_TILE, GE_TILE + 1, (1 << 13) + 3])
def test_evaluate(n):
    stride, words, t = eval_case(n)
    points = [edge_point(k) for k in range(GE_PTS + 1)]
    got = E.evaluate_device(t, 3, n, points, stride)
    assert got.shape == (3, GE_PTS + 1, 2)
    for k in range(3):
        col = words[k * stride:k * stride + n].tolist()
        for j, z in enumerate(points):
            assert tuple(got[k, j].tolist()) == X.horner(col, z), (k, j)


@pytest.mark.parametrize("m", [1, 2])
def test_evaluate_fewer_points_and_an_ext_polynomial(m):
    n = GE_TILE + 1
    stride, words, t = eval_case(n)
    points = [edge_point(9 + k) for k in range(m)]
    got = E.evaluate_device(t, 3, n, points, stride)
    for k in range(3):
        for j, z in enumerate(points):
            assert tuple(got[k, j].tolist()) == X.horner(words[k * stride:k * stride + n].tolist(), z)
    # columns 0 and 1 as the planes of one polynomial over Fp2
    coeffs = [X.elem(c) for c in zip(words[:n].tolist(), words[stride:stride + n].tolist())]
    assert E.evaluate_ext_device(t, n, points, stride) == [X.horner_ext(coeffs, z) for z in points]


def test_evaluate_two_tile_sums_per_work_item():
    n = 256 * GE_TILE + 5   # 257 tiles: the fold kernel's work-items take two tile sums each
    words = rand_words(n, 59)
    z = (G.EDGE[20], G.EDGE[27])
    got = E.evaluate_device(dev(words), 1, n, [z])
    assert tuple(got[0, 0].tolist()) == X.horner(words.tolist(), z)


def test_evaluate_more_columns_than_the_grids_y_extent():
    k = 65537   # two launches per kernel: columns 0 .. 65534, then 65535 and 65536
    words = rand_words(2 * k, 58)
    z = edge_point(3)
    got = E.evaluate_device(dev(words), k, 2, [z], 2)
    assert got.shape == (k, 1, 2)
    assert [tuple(v) for v in got[:, 0].tolist()] == [X.horner(c, z) for c in words.reshape(k, 2).tolist()]


# ---- DEEP quotients
def deep_case(log2t, blowup, m, seed, h=7, root=G.OTHER_ROOT):
    T, log2n = 1 << log2t, log2t + blowup.bit_length() - 1
    coeffs = rand_words((3, T), seed) % np.uint64(P)
    stride = (1 << log2n) + 8
    t_lde = empty(3 * stride)
    goldilocks.lde_device(dev(coeffs), log2t, t_lde, log2n, batch=3, out_stride=stride, offset=h, root=root)
    points = rand_elems(m, seed + 1)
    weights = [rand_elems(m, seed + 2 + k) for k in range(3)]
    weights[1][m - 1] = (0, 0)                                  # a zero weight
    evals = [[X.horner(coeffs[k].tolist(), z) for z in points] for k in range(3)]
    return T, log2n, coeffs, stride, t_lde, points, weights, evals, h, root


def deep_run(case, evals=None, out_stride=0):
    T, log2n, _, stride, t_lde, points, weights, true_evals, h, root = case
    n = 1 << log2n
    t_out = empty((out_stride or n) + n)
    E.deep_quotients_device(t_lde, 3, log2n, points, weights, evals or true_evals, t_out, stride, out_stride, offset=h, root=root)
    return t_out


@pytest.mark.parametrize("log2t,blowup", [(1, 2), (1, 4), (4, 2), (4, 4), (10, 2), (10, 4)])
def test_deep_quotients(log2t, blowup):
    case = deep_case(log2t, blowup, 2, 60 + log2t + blowup)
    T, log2n, coeffs, stride, t_lde, points, weights, evals, h, root = case
    n = 1 << log2n
    cols = host(t_lde).reshape(3, stride)[:, :n]
    assert np.array_equal(cols, G.np_evaluate_fft(coeffs, h, root, log2n=log2n))
    # every row against the definition
    out_stride = n + 24
    t_out = deep_run(case, out_stride=out_stride)
    got = host(t_out)
    assert elems_of((got[:n], got[out_stride:])) == X.deep_rows(cols.tolist(), log2n, h, root, points, weights, evals)
    # with the true values the quotient is a polynomial of degree < T - 1: the coefficients from T - 1 on are zero
    t_q = deep_run(case)
    goldilocks.ntt_device(t_q, t_q, log2n, inverse=True, batch=2, offset=h, root=root)
    q = host(t_q).reshape(2, n)
    assert not q[:, T - 1:].any() and (T == 2 or q[:, :T - 1].any())
    # ... and with one value off by one they are not
    wrong = [list(row) for row in evals]
    wrong[2][0] = ((wrong[2][0][0] + 1) % P, wrong[2][0][1])
    t_q = deep_run(case, wrong)
    goldilocks.ntt_device(t_q, t_q, log2n, inverse=True, batch=2, offset=h, root=root)
    assert host(t_q).reshape(2, n)[:, T - 1:].any()


def test_deep_quotients_more_points_than_a_launch_and_fewer_rows_than_a_work_item():
    case = deep_case(4, 4, GD_PTS + 1, 71, h=P - 3, root=G.ROOT)
    T, log2n, _, stride, t_lde, points, weights, evals, h, root = case
    n = 1 << log2n
    cols = host(t_lde).reshape(3, stride)[:, :n]
    got = host(deep_run(case)).reshape(2, n)
    assert elems_of(got) == X.deep_rows(cols.tolist(), log2n, h, root, points, weights, evals)
    # a domain of GD_ROWS / 2 rows, no offset, any columns
    cols = rand_words((3, 2), 72)
    t_out = empty(4)
    E.deep_quotients_device(dev(cols), 3, 1, points[:2], [w[:2] for w in weights], [e[:2] for e in evals], t_out)
    assert elems_of(host(t_out).reshape(2, 2)) == X.deep_rows(cols.tolist(), 1, 1, G.ROOT, points[:2], [w[:2] for w in weights], [e[:2] for e in evals])
    # an Fp2 column as its two planes: weights w and t w
    w = rand_elems(2, 73)
    e = rand_elems(2, 74)
    rows_w, rows_tw = E.plane_weights(w)
    e0, e1 = [(x[0], 0) for x in e], [(x[1], 0) for x in e]
    E.deep_quotients_device(dev(cols), 2, 1, points[:2], [rows_w, rows_tw], [e0, e1], t_out)
    c = [X.elem((cols[0][i], cols[1][i])) for i in range(2)]
    want = []
    for i in range(2):
        x = (pow(G.root_of_unity(1), i, P), 0)
        want.append(X.add(*[X.mul(X.mul(w[j], X.sub(c[i], e[j])), X.inv(X.sub(x, points[j]))) for j in range(2)]))
    assert elems_of(host(t_out).reshape(2, 2)) == want


# ---- one FRI layer
_LAYER_IN = {}


def layer_input(n):
    if n not in _LAYER_IN:
        stride = n + 6
        words = rand_words(stride + n, 80 + n % 89)
        words[0], words[stride + n - 1] = P, (1 << 64) - 1
        coeffs = [X.elem(c) for c in zip(words[:n].tolist(), words[stride:].tolist())]
        _LAYER_IN[n] = (stride, dev(words), coeffs)
    return _LAYER_IN[n]


ZETA = (G.EDGE[26], G.EDGE[13])
LAYER_CASES = [(1, 2), (2, 2), (3, 2), (3, 4), (5, 4), (5, 1 << 10), ((1 << 9) + 1, 1 << 10), ((1 << 9) + 1, 1 << 11), (1 << 12, 1 << 11),
               (1 << 12, 1 << 13)]


@pytest.mark.parametrize("level", LEVELS)
@pytest.mark.parametrize("n,domain", LAYER_CASES)
def test_fri_layer(n, domain, level):
    stride, t_coeffs, coeffs = layer_input(n)
    h, root = (1 << 32) + 5, G.OTHER_ROOT if domain == 1 << 10 else 0
    t_poly, t_eval, t_nodes, out_root = E.fri_layer_device(t_coeffs, n, ZETA, h, domain, level, coeff_stride=stride, root=root)
    block = X.fold(coeffs, ZETA)
    assert len(block) == E.folded_block(n) == t_poly.numel() // 2
    assert elems_of(host(t_poly).reshape(2, -1)) == block          # the zero padding included
    planes = X.np_layer_evaluation(block, domain, h, root or G.ROOT)
    got = host(t_eval).reshape(2, domain)
    assert np.array_equal(got, planes)
    if domain <= 4:
        assert elems_of(got) == X.layer_evaluation(block, domain, h)
    nodes = X.layer_tree(level, planes)
    assert nodes.shape == (domain - 1, E.digest_words(level))
    assert np.array_equal(host(t_nodes).reshape(nodes.shape), nodes)   # every node
    assert np.array_equal(out_root, nodes[0])
    # leaf 1 (or 0) from the definition: the four words (a.c0, a.c1, b.c0, b.c1), element after element
    j = 1 if domain > 2 else 0
    i = X.pair_index(j, domain)
    assert nodes[domain // 2 - 1 + j].tolist() == R.hash(level, [int(got[0, i]), int(got[1, i]), int(got[0, i + domain // 2]), int(got[1, i + domain // 2])])


@pytest.mark.parametrize("n", [1, 2, 5, (1 << 9) + 1])
def test_fri_fold_only(n):
    stride, t_coeffs, coeffs = layer_input(n)
    t_poly, t_eval, t_nodes, out_root = E.fri_layer_device(t_coeffs, n, ZETA, None, 0, coeff_stride=stride, fold_only=True)
    assert t_eval is None and t_nodes is None and out_root is None
    assert elems_of(host(t_poly).reshape(2, -1)) == X.fold(coeffs, ZETA)


def test_fri_fold_identity_between_consecutive_layers():
    n, N, h = (1 << 9) + 1, 1 << 11, 7
    stride, t_coeffs, _ = layer_input(n)
    t_p1, t_e1, _, _ = E.fri_layer_device(t_coeffs, n, ZETA, h, N, coeff_stride=stride)
    zeta2 = (G.EDGE[11], G.EDGE[24])
    _, t_e2, _, _ = E.fri_layer_device(t_p1, E.folded_block(n), zeta2, h * h % P, N // 2)   # the dense block is the next polynomial
    e1, e2 = elems_of(host(t_e1).reshape(2, N)), elems_of(host(t_e2).reshape(2, N // 2))
    w = G.root_of_unity(11)
    x_inv = pow(h, P - 2, P)
    w_inv = pow(w, P - 2, P)
    for i in range(N // 2):
        a, b = e1[i], e1[i + N // 2]
        assert e2[i] == X.add(X.add(a, b), X.mul(zeta2, X.mul_base(X.sub(a, b), x_inv))), i
        x_inv = x_inv * w_inv % P


# ---- the commit phase
def test_fri_commit_phase():
    n, domain, h, layers_n, level = 1 << 10, 1 << 12, 7, 10, E.RPO_128
    planes = rand_words((2, n), 90)
    coeffs = [X.elem(c) for c in elems_of(planes)]
    zetas = rand_elems(layers_n, 91)
    seen, feed = [], list(zetas)

    def challenge(prev_root):
        seen.append(None if prev_root is None else prev_root.tolist())
        return feed.pop(0)

    last, layers = E.fri_commit_phase_device(dev(planes), n, layers_n, h, domain, challenge, level)
    want_last, want_layers = X.commit_phase(coeffs, layers_n, h, domain, zetas, level)
    assert last == want_last and not feed
    assert len(layers) == len(want_layers) == layers_n - 1
    for (t_eval, t_nodes, root), (w_planes, w_nodes) in zip(layers, want_layers):
        assert np.array_equal(root, w_nodes[0])
        assert np.array_equal(host(t_eval).reshape(w_planes.shape), w_planes)
        assert np.array_equal(host(t_nodes).reshape(w_nodes.shape), w_nodes)
    assert seen == [None] + [w_nodes[0].tolist() for _, w_nodes in want_layers]
    # the constant: the last polynomial has one coefficient, the value of the folds all the way down
    assert domain >> (layers_n - 1) == 8 and want_layers[-1][0].shape == (2, 8)
    # layer 0 opens through the existing call: 32-byte nodes, no columns
    t_eval, t_nodes, root = layers[0]
    N = domain // 2
    ev = host(t_eval).reshape(2, N)
    log2_leaves = N.bit_length() - 2
    positions = [0, N // 2 - 1] + [int(x) for x in np.random.default_rng(92).integers(0, N // 2, 6)]
    tree = merkle.Tree(fft.Stark252PrimeField, t_nodes, log2_leaves)
    _, paths = merkle.open_trees_device([tree], np.array(positions, np.uint64))
    assert paths[0].shape == (len(positions), log2_leaves, 32)
    for q, pos in enumerate(positions):
        i = X.pair_index(pos, N)
        cur = R.hash(level, [int(ev[0, i]), int(ev[1, i]), int(ev[0, i + N // 2]), int(ev[1, i + N // 2])])
        k = pos
        for sib in paths[0][q].view(np.uint64).reshape(log2_leaves, 4).tolist():
            cur = R.hash(level, cur + sib) if k % 2 == 0 else R.hash(level, sib + cur)
            k >>= 1
        assert cur == root.tolist(), pos
