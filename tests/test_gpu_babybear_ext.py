"""The BabyBear quartic extension on the device (csrc/babybear_ext.cuh, babybear_ext.hip) against the model of
tests/babybear_ext_ref.py, bit for bit: the pointwise seam at the operand edges, the layout bridge, out-of-domain
evaluation, the DEEP quotients, one FRI layer, and one pipeline from the LDE to the last FRI value.

The device holds STORED words (v 2^32 mod p), the model residues: X.np_store / X.np_unstore sit between them.

Launch boundaries (the constants of babybear_ext.hip): evaluate gives a work-item BE_E = 8 coefficients and a block
BE_TILE = 2048; the fold kernel gives a work-item one tile sum up to 256 tiles and two from 2^19 + 1 coefficients on; a
launch holds BE_PTS = 4 points.  DEEP gives a work-item BD_ROWS = 4 rows and a launch BD_PTS = 4 points.  The layer's
tree builds its first levels inside the leaf kernel from 2^10 to 2^16 leaves, that is on the domains 2^11 .. 2^17; above
that the leaf kernel hands its leaves out in tiles (domain 2^18: the one case of that size, on a block of 4 coefficients)."""
import numpy as np
import pytest
import torch

from lambda_elliptic_curves_amd import babybear_ext as E
from lambda_elliptic_curves_amd import fft, merkle
from oracle import oracle as O
from tests import babybear_ext_ref as X

pytestmark = pytest.mark.gpu
P = X.P
BE_E, BE_TILE, BE_PTS, BD_ROWS, BD_PTS = 8, 2048, 4, 4, 4
U32 = fft.Babybear31PrimeFieldU32


def dev(a):
    return torch.from_numpy(np.array(a, dtype=np.uint32, order="C").view(np.int32)).cuda()


def host(t):
    return t.cpu().numpy().view(np.uint32)


def empty(n, fill=0):
    return torch.full((n,), fill, dtype=torch.int32, device="cuda")


def rand_res(shape, seed):
    """residues below p"""
    return np.random.default_rng(seed).integers(0, P, shape).astype(np.uint64)


def rand_elems(n, seed):
    return [tuple(int(v) for v in row) for row in rand_res((n, 4), seed)]


def grid4(words):
    w = np.array(words, np.uint64)
    return np.stack([g.reshape(-1) for g in np.meshgrid(w, w, w, w, indexing="ij")])


def stored(elems):
    """model elements -> the host scalars of the calls"""
    return [X.store_elem(e) for e in elems]


def edge_point(k):
    """a point whose stored words come from the edge set, c3 != 0"""
    ed = X.EDGE
    return X.unstore_elem((ed[(3 * k + 1) % 8], ed[(5 * k + 2) % 8], ed[(k + 3) % 8], ed[(7 * k + 5) % 8] or 1))


# ---- pointwise
def test_pointwise_mul_on_the_edge_operands():
    ea, eb = grid4(X.EDGE), grid4(X.EDGE_B)                 # stored words
    na, nb = ea.shape[1], eb.shape[1]
    a, b = np.repeat(ea, nb, axis=1), np.tile(eb, (1, na))
    n = a.shape[1]
    assert n == 1 << 20
    both = np.flatnonzero((a == P - 1).all(axis=0) & (b == P - 1).all(axis=0))
    assert both.size == 1                                   # the all-(p - 1) pair is among them
    t_out = empty(4 * n)
    E.pointwise_device(E.MUL, dev(a), dev(b), t_out, n)
    got = host(t_out).reshape(4, n)
    want = X.np_store(X.np_mul(X.np_unstore(a), X.np_unstore(b)))
    assert np.array_equal(got, want)
    for i in (int(both[0]), 123457):
        assert tuple(got[:, i].tolist()) == X.store_elem(X.mul(X.unstore_elem(a[:, i]), X.unstore_elem(b[:, i])))


def test_pointwise_sqr_inv_and_mul_base():
    a = np.concatenate([grid4(X.EDGE), X.np_store(rand_res((4, 1 << 12), 41))], axis=1)
    a[:, 4096 + 2] = 0
    n = a.shape[1]
    elems = X.elems_of(X.np_unstore(a))
    t_a, t_out = dev(a), empty(4 * n)
    E.pointwise_device(E.SQR, t_a, None, t_out, n)
    assert np.array_equal(host(t_out).reshape(4, n), X.np_store(X.planes_of([X.sqr(e) for e in elems])))
    E.pointwise_device(E.INV, t_a, None, t_out, n)
    inv = X.elems_of(X.np_unstore(host(t_out).reshape(4, n)))
    assert (host(t_out) < P).all() and inv == [X.inv(e) for e in elems]
    assert inv[0] == X.ZERO and inv[4096 + 2] == X.ZERO        # the inverse of zero is written as zero
    assert all(X.mul(e, v) == X.ONE for e, v in zip(elems, inv) if e != X.ZERO)
    # a b with b in F: every edge word against E^4, random words against the random elements
    b = np.concatenate([np.tile(np.array(X.EDGE, np.uint64), 512), X.np_store(rand_res(1 << 12, 42))])
    E.pointwise_device(E.MUL_BASE, t_a, dev(b), t_out, n)
    assert np.array_equal(host(t_out).reshape(4, n), X.np_store(X.np_mul_base(X.np_unstore(a), X.np_unstore(b))))
    a8 = np.repeat(grid4(X.EDGE), 8, axis=1)                   # E^4 x E in full
    b8 = np.tile(np.array(X.EDGE, np.uint64), 4096)
    t_out = empty(4 * b8.size)
    E.pointwise_device(E.MUL_BASE, dev(a8), dev(b8), t_out, b8.size)
    assert np.array_equal(host(t_out).reshape(4, -1), X.np_store(X.np_mul_base(X.np_unstore(a8), X.np_unstore(b8))))


def strided(words, n, stride):
    return np.stack([words[e * stride:e * stride + n] for e in range(4)])


def test_pointwise_strides_in_place_and_one_element():
    n, sa, sb, so = 1000, 1003, 1024, 1501
    a, b = X.np_store(rand_res(3 * sa + n, 43)), X.np_store(rand_res(3 * sb + n, 44))
    want = X.np_store(X.np_mul(X.np_unstore(strided(a, n, sa)), X.np_unstore(strided(b, n, sb))))
    t_out = empty(3 * so + n, 0x5555)
    E.pointwise_device(E.MUL, dev(a), dev(b), t_out, n, sa, sb, so)
    got = host(t_out)
    assert np.array_equal(strided(got, n, so), want)
    assert all((got[e * so + n:(e + 1) * so] == 0x5555).all() for e in range(3))   # the words between the planes are not touched
    # in place, over a and over b
    t_a, t_b = dev(a), dev(b)
    E.pointwise_device(E.MUL, t_a, t_b, t_a, n, sa, sb, sa)
    got = host(t_a)
    assert np.array_equal(strided(got, n, sa), want)
    assert all(np.array_equal(got[e * sa + n:(e + 1) * sa], a[e * sa + n:(e + 1) * sa]) for e in range(3))
    t_a = dev(a)
    E.pointwise_device(E.MUL, t_a, t_b, t_b, n, sa, sb, sb)
    assert np.array_equal(strided(host(t_b), n, sb), want)
    t_a = dev(a)
    E.pointwise_device(E.INV, t_a, None, t_a, n, sa, 0, sa)
    assert X.elems_of(X.np_unstore(strided(host(t_a), n, sa))) == [X.inv(e) for e in X.elems_of(X.np_unstore(strided(a, n, sa)))]
    # one element
    x, y = (P - 2, 5, 0, P - 1), (P - 1, 3, 7, 1)
    for op, f in ((E.MUL, X.mul), (E.SQR, lambda u, _: X.sqr(u)), (E.INV, lambda u, _: X.inv(u)), (E.MUL_BASE, lambda u, v: X.mul_base(u, v[0]))):
        t_out = empty(4)
        E.pointwise_device(op, dev(X.store_elem(x)), dev(X.store_elem(y)), t_out, 1)
        assert tuple(host(t_out).tolist()) == X.store_elem(f(x, y))


# ---- the bridge to the interleaved layout
@pytest.mark.parametrize("n", [1, 255, 256, (1 << 12) + 3])
def test_convert_round_trip(n):
    planes = X.np_store(rand_res((4, n), 45 + n % 7))
    planes[:, 0] = [0, P - 1, 1, X.R % P]
    stride = n + 5
    padded = np.full(3 * stride + n, 0x5555, np.uint32)
    for e in range(4):
        padded[e * stride:e * stride + n] = planes[e]
    # bb_to_r64 in Python: the stored word w stands for w 2^-32, its u64 word is that times 2^64
    inter = (planes.astype(np.uint64) << np.uint64(32)) % np.uint64(P)
    want = np.ascontiguousarray(inter.T).reshape(-1)          # element after element, four u64 words each
    t_inter = torch.zeros(4 * n, dtype=torch.int64, device="cuda")
    E.to_interleaved_device(dev(padded), t_inter, n, stride)
    assert np.array_equal(t_inter.cpu().numpy().view(np.uint64), want)
    t_planes = empty(3 * stride + n, 0x7777)
    E.to_planes_device(t_inter, t_planes, n, stride)
    got = host(t_planes)
    assert np.array_equal(strided(got, n, stride), planes)
    assert all((got[e * stride + n:(e + 1) * stride] == 0x7777).all() for e in range(3))
    t_dense = empty(4 * n)
    E.to_planes_device(t_inter, t_dense, n)
    assert np.array_equal(host(t_dense).reshape(4, n), planes)


# ---- evaluate
_EVAL = {}


def eval_case(n):
    """3 columns of n coefficients (residues), 16 words of other data between two columns; shared by the cases of one length"""
    if n not in _EVAL:
        stride = n + 16
        res = rand_res(3 * stride, 50 + n % 97)
        res[0], res[min(1, n - 1)] = P - 1, X.unstore(P - 1)
        _EVAL[n] = (stride, res, dev(X.np_store(res)))
    return _EVAL[n]


def horner(col, z):
    return X.horner(col.tolist(), z) if len(col) <= 64 else X.np_horner(col, z)   # (the two agree: tests/test_babybear_ext_cpu.py)


@pytest.mark.parametrize("n", [1, 2, 3, BE_E - 1, BE_E, BE_E + 1, BE_TILE - 1, BE_TILE, BE_TILE + 1, (1 << 13) + 3])
def test_evaluate(n):
    stride, res, t = eval_case(n)
    points = [edge_point(k) for k in range(BE_PTS + 1)]        # more than one launch takes
    got = E.evaluate_device(t, 3, n, stored(points), stride)
    assert got.shape == (3, BE_PTS + 1, 4)
    for k in range(3):
        col = res[k * stride:k * stride + n]
        for j, z in enumerate(points):
            assert tuple(got[k, j].tolist()) == X.store_elem(horner(col, z)), (k, j)


@pytest.mark.parametrize("m", [1, 2])
def test_evaluate_fewer_points_and_an_ext_polynomial(m):
    n = BE_TILE + 1
    stride, res, _ = eval_case(n)
    res4 = np.concatenate([res, rand_res(stride, 58)])           # a fourth plane
    t = dev(X.np_store(res4))
    points = [edge_point(9 + k) for k in range(m)]
    got = E.evaluate_device(t, 3, n, stored(points), stride)
    for k in range(3):
        for j, z in enumerate(points):
            assert tuple(got[k, j].tolist()) == X.store_elem(horner(res4[k * stride:k * stride + n], z))
    # the four columns as the planes of one polynomial over Fp4
    coeffs = X.elems_of(strided(res4, n, stride))
    assert E.evaluate_ext_device(t, n, stored(points), stride) == stored([X.horner_ext(coeffs, z) for z in points])


def test_evaluate_two_tile_sums_per_work_item():
    n = 256 * BE_TILE + 5   # 257 tiles: the fold kernel's work-items take two tile sums each
    res = rand_res(n, 59)
    z = edge_point(4)
    got = E.evaluate_device(dev(X.np_store(res)), 1, n, stored([z]))
    assert tuple(got[0, 0].tolist()) == X.store_elem(X.np_horner(res, z))
    assert E.evaluate_device(dev(X.np_store(res)), 1, 0, stored([z])).tolist() == [[[0, 0, 0, 0]]]   # n_coeffs = 0: zeros


def test_evaluate_more_columns_than_the_grids_y_extent():
    k = 65537   # two launches per kernel: columns 0 .. 65534, then 65535 and 65536
    res = rand_res(2 * k, 57)
    z = edge_point(3)
    got = E.evaluate_device(dev(X.np_store(res)), k, 2, stored([z]), 2)
    assert got.shape == (k, 1, 4)
    assert [tuple(v) for v in got[:, 0].tolist()] == [X.store_elem(X.horner(c, z)) for c in res.reshape(k, 2).tolist()]


# ---- DEEP quotients
def deep_case(log2t, blowup, m, seed, h):
    T, log2n = 1 << log2t, log2t + blowup.bit_length() - 1
    n = 1 << log2n
    coeffs = rand_res((3, T), seed)
    t_dense = empty(3 * n)
    fft.lde_device(U32, dev(X.np_store(coeffs)), log2t, t_dense, log2n, batch=3, offset=np.array([X.store(h)], np.uint32))
    stride = n + 8
    t_lde = empty(3 * stride, 0x1234)
    t_lde.view(3, stride)[:, :n] = t_dense.view(3, n)
    points = rand_elems(m, seed + 1)
    weights = [rand_elems(m, seed + 2 + k) for k in range(3)]
    weights[1][m - 1] = X.ZERO                                  # a zero weight
    evals = [[X.np_horner(coeffs[k], z) for z in points] for k in range(3)]
    return T, log2n, coeffs, stride, t_lde, points, weights, evals, h


def deep_run(case, evals=None, out_stride=0):
    T, log2n, _, stride, t_lde, points, weights, true_evals, h = case
    n = 1 << log2n
    t_out = empty(3 * (out_stride or n) + n, 0x4321)
    E.deep_quotients_device(t_lde, 3, log2n, stored(points), [stored(r) for r in weights], [stored(r) for r in (evals or true_evals)], t_out,
                            stride, out_stride, offset=X.store(h))
    return t_out


def coefficients_of(t_q, log2n, h):
    """inverse coset transform of an Fp4 vector in dense planes -> (4, n) stored words"""
    t_c = torch.empty_like(t_q)
    fft.ntt_device(U32, t_q, t_c, log2n, inverse=True, batch=4, offset=np.array([X.store(h)], np.uint32))
    return host(t_c).reshape(4, -1)


@pytest.mark.parametrize("log2t,blowup,h", [(1, 2, 7), (1, 4, P - 1), (4, 2, P - 1), (4, 4, 7), (10, 2, 7), (10, 4, P - 1)])
def test_deep_quotients(log2t, blowup, h):
    case = deep_case(log2t, blowup, 2, 60 + log2t + blowup, h)
    T, log2n, coeffs, stride, t_lde, points, weights, evals, _ = case
    n = 1 << log2n
    cols = X.np_unstore(host(t_lde).reshape(3, stride)[:, :n])
    assert np.array_equal(cols, X.np_lde(coeffs, log2n, h))
    # every row against the definition
    out_stride = n + 24
    got = host(deep_run(case, out_stride=out_stride))
    assert X.elems_of(X.np_unstore(strided(got, n, out_stride))) == X.deep_rows(cols.tolist(), log2n, h, points, weights, evals)
    assert all((got[e * out_stride + n:(e + 1) * out_stride] == 0x4321).all() for e in range(3))
    # with the true values the quotient is a polynomial of degree < T - 1: the coefficients from T - 1 on are zero
    q = coefficients_of(deep_run(case), log2n, h)
    assert not q[:, T - 1:].any() and (T == 2 or q[:, :T - 1].any())
    # ... and with one value off by one they are not
    wrong = [list(row) for row in evals]
    wrong[2][0] = ((wrong[2][0][0] + 1) % P,) + wrong[2][0][1:]
    assert coefficients_of(deep_run(case, wrong), log2n, h)[:, T - 1:].any()


def test_deep_quotients_more_points_than_a_launch_and_fewer_rows_than_a_work_item():
    case = deep_case(4, 4, BD_PTS + 1, 71, P - 3)
    T, log2n, _, stride, t_lde, points, weights, evals, h = case
    n = 1 << log2n
    cols = X.np_unstore(host(t_lde).reshape(3, stride)[:, :n])
    got = host(deep_run(case)).reshape(4, n)
    assert X.elems_of(X.np_unstore(got)) == X.deep_rows(cols.tolist(), log2n, h, points, weights, evals)
    # a domain of BD_ROWS / 2 rows, no offset, any columns
    cols = rand_res((3, 2), 72)
    w2, e2 = [w[:2] for w in weights], [e[:2] for e in evals]
    t_out = empty(8)
    E.deep_quotients_device(dev(X.np_store(cols)), 3, 1, stored(points[:2]), [stored(r) for r in w2], [stored(r) for r in e2], t_out)
    assert X.elems_of(X.np_unstore(host(t_out).reshape(4, 2))) == X.deep_rows(cols.tolist(), 1, 1, points[:2], w2, e2)
    # an Fp4 column as its four planes: weights w, x w, x^2 w, x^3 w
    cols = rand_res((4, 2), 73)
    w, e = rand_elems(2, 74), rand_elems(2, 75)
    rows = E.plane_weights(stored(w))
    plane_evals = [[X.store_elem((x[k], 0, 0, 0)) for x in e] for k in range(4)]
    E.deep_quotients_device(dev(X.np_store(cols)), 4, 1, stored(points[:2]), rows, plane_evals, t_out)
    c = X.elems_of(cols)
    want = []
    for i in range(2):
        x = (pow(X.root_of_unity(1), i, P), 0, 0, 0)
        want.append(X.add(*[X.mul(X.mul(w[j], X.sub(c[i], e[j])), X.inv(X.sub(x, points[j]))) for j in range(2)]))
    assert X.elems_of(X.np_unstore(host(t_out).reshape(4, 2))) == want


# ---- one FRI layer
_LAYER_IN = {}


def layer_input(n):
    if n not in _LAYER_IN:
        stride = n + 6
        res = rand_res(3 * stride + n, 80 + n % 89)
        res[0], res[3 * stride + n - 1] = P - 1, X.unstore(P - 1)
        _LAYER_IN[n] = (stride, dev(X.np_store(res)), X.elems_of(strided(res, n, stride)))
    return _LAYER_IN[n]


ZETA = X.unstore_elem((X.EDGE[3], X.EDGE[6], X.EDGE[4], X.EDGE[7]))
LAYER_CASES = [(1, 2), (2, 2), (3, 2), (3, 4), (5, 4), (5, 1 << 10), ((1 << 9) + 1, 1 << 10), ((1 << 9) + 1, 1 << 11), (1 << 12, 1 << 11),
               (1 << 12, 1 << 14), (5, 1 << 18)]


@pytest.mark.parametrize("n,domain", LAYER_CASES)
def test_fri_layer(n, domain):
    stride, t_coeffs, coeffs = layer_input(n)
    h = P - 5 if domain == 1 << 10 else 49
    t_poly, t_eval, t_nodes, out_root = E.fri_layer_device(t_coeffs, n, X.store_elem(ZETA), X.store(h), domain, coeff_stride=stride)
    block = X.fold(coeffs, ZETA)
    assert len(block) == E.folded_block(n) == t_poly.numel() // 4
    assert X.elems_of(X.np_unstore(host(t_poly).reshape(4, -1))) == block          # the zero padding included
    planes = X.np_layer_evaluation(block, domain, h)
    got = host(t_eval).reshape(4, domain)
    assert np.array_equal(got, X.np_store(planes))
    if domain <= 4:
        assert X.elems_of(X.np_unstore(got)) == X.layer_evaluation(block, domain, h)
    nodes = X.layer_tree(planes)
    assert nodes.shape == (domain - 1, 32)
    assert np.array_equal(t_nodes.cpu().numpy(), nodes)              # every node
    assert np.array_equal(out_root, nodes[0])
    # leaf 1 (or 0) from the definition: the eight words a.c0 .. a.c3, b.c0 .. b.c3, big-endian
    j = 1 if domain > 2 else 0
    i = X.pair_index(j, domain)
    assert nodes[domain // 2 - 1 + j].tobytes() == X.leaf_hash(list(got[:, i]) + list(got[:, i + domain // 2]))


@pytest.mark.parametrize("n", [1, 2, 5, (1 << 9) + 1])
def test_fri_fold_only(n):
    stride, t_coeffs, coeffs = layer_input(n)
    t_poly, t_eval, t_nodes, out_root = E.fri_layer_device(t_coeffs, n, X.store_elem(ZETA), None, 0, coeff_stride=stride, fold_only=True)
    assert t_eval is None and t_nodes is None and out_root is None
    assert X.elems_of(X.np_unstore(host(t_poly).reshape(4, -1))) == X.fold(coeffs, ZETA)


def verify_opening(path, leaf, pos, root):
    cur, k = leaf, pos
    for sib in path:
        cur = O.keccak256(cur + sib.tobytes()) if k % 2 == 0 else O.keccak256(sib.tobytes() + cur)
        k >>= 1
    return cur == root


# ---- the pipeline: LDE -> commitment -> OOD -> DEEP -> coefficients -> FRI commit phase
def test_pipeline_from_the_lde_to_the_last_fri_value():
    log2t, blowup, n_cols, h, layers_n = 10, 4, 4, 7, 10
    T, log2n = 1 << log2t, log2t + 2
    N = 1 << log2n
    off = np.array([X.store(h)], np.uint32)
    trace = rand_res((n_cols, T), 90)
    t_lde = empty(n_cols * N)
    fft.lde_device(U32, dev(X.np_store(trace)), log2t, t_lde, log2n, batch=n_cols, offset=off)
    cols = X.np_lde(trace, log2n, h)
    assert np.array_equal(host(t_lde).reshape(n_cols, N), X.np_store(cols))
    t_tree = torch.zeros((2 * N - 1, 32), dtype=torch.uint8, device="cuda")
    root = merkle.commit_columns_layout_device(U32, t_lde, n_cols, log2n, t_tree)
    assert root == O.merkle_commit_columns_babybear(X.np_store(cols))[0].tobytes()
    # out-of-domain values at z and z g, g the generator of the trace domain
    z = rand_elems(1, 91)[0]
    points = [z, X.mul_base(z, X.root_of_unity(log2t))]
    t_trace = dev(X.np_store(trace))
    ood = E.evaluate_device(t_trace, n_cols, T, stored(points))
    evals = [[X.np_horner(trace[k], p) for p in points] for k in range(n_cols)]
    assert ood.tolist() == [[list(X.store_elem(v)) for v in row] for row in evals]
    # DEEP quotients over the LDE domain and their coefficients
    weights = [rand_elems(2, 92 + k) for k in range(n_cols)]
    t_deep = empty(4 * N)
    E.deep_quotients_device(t_lde, n_cols, log2n, stored(points), [stored(r) for r in weights], [[tuple(v) for v in row] for row in ood.tolist()],
                            t_deep, offset=X.store(h))
    deep = X.np_unstore(host(t_deep).reshape(4, N))
    rows = list(range(0, N, 97)) + [N - 1]
    assert [tuple(int(v) for v in deep[:, i]) for i in rows] == X.deep_rows(cols.tolist(), log2n, h, points, weights, evals, rows)
    q = X.np_unstore(coefficients_of(t_deep, log2n, h))
    assert not q[:, T - 1:].any() and q[:, :T - 1].any()           # degree < T - 1: no model involved
    assert np.array_equal(X.np_lde(q[:, :T], log2n, h), deep)      # the model's transform of those coefficients: every row
    # the FRI commit phase on the T coefficients
    t_q = dev(X.np_store(q[:, :T]))
    zetas = rand_elems(layers_n, 96)
    seen, feed = [], list(zetas)

    def challenge(prev_root):
        seen.append(None if prev_root is None else prev_root.tobytes())
        return X.store_elem(feed.pop(0))

    last, layers = E.fri_commit_phase_device(t_q, T, layers_n, X.store(h), N, challenge)
    want_last, want_layers = X.commit_phase(X.elems_of(q[:, :T]), layers_n, h, N, zetas)
    assert last == X.store_elem(want_last) and not feed
    assert len(layers) == len(want_layers) == layers_n - 1
    for (t_eval, t_nodes, layer_root), (w_planes, w_nodes) in zip(layers, want_layers):
        assert np.array_equal(layer_root, w_nodes[0])
        assert np.array_equal(host(t_eval).reshape(w_planes.shape), X.np_store(w_planes))
        assert np.array_equal(t_nodes.cpu().numpy(), w_nodes)
    assert seen == [None] + [w_nodes[0].tobytes() for _, w_nodes in want_layers]
    assert N >> (layers_n - 1) == 8 and want_layers[-1][0].shape == (4, 8)
    # layer 0 opens through the existing call: 32-byte nodes, no columns
    t_eval, t_nodes, layer_root = layers[0]
    D = N // 2
    ev = host(t_eval).reshape(4, D)
    log2_leaves = D.bit_length() - 2
    positions = [0, D // 2 - 1] + [int(x) for x in np.random.default_rng(97).integers(0, D // 2, 6)]
    tree = merkle.Tree(fft.Stark252PrimeField, t_nodes, log2_leaves)
    _, paths = merkle.open_trees_device([tree], np.array(positions, np.uint64))
    assert paths[0].shape == (len(positions), log2_leaves, 32)
    for k, pos in enumerate(positions):
        i = X.pair_index(pos, D)
        leaf = X.leaf_hash(list(ev[:, i]) + list(ev[:, i + D // 2]))
        assert verify_opening(paths[0][k], leaf, pos, want_layers[0][1][0].tobytes()), pos
