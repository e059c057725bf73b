"""The quartic extension of Mersenne31 on the device (csrc/mersenne31_ext.cuh, mersenne31_ext.hip) against the model of
tests/mersenne31_ext_ref.py, bit for bit: the pointwise seam at the word edges, out-of-domain evaluation, the DEEP quotients
by lines, the circle FRI fold with its layer trees, and one chain from the LDE to a constant last layer.

Launch boundaries (the constants of mersenne31_ext.cuh): evaluate gives a work-item 8 coefficients and a block 2^11; every
further launch folds 256 sums, so 2^16 coefficients are 32 tile sums in one fold launch; a launch holds 4 points.  DEEP
gives a work-item 4 rows (a block 2^10 rows) and a launch 4 points, and takes the columns two at a time."""
import numpy as np
import pytest
import torch

from lambda_elliptic_curves_amd import circle, fft, merkle, monolith
from lambda_elliptic_curves_amd import mersenne31_ext as E
from tests import circle_ref as CR
from tests import mersenne31_ext_ref as R
from tests import monolith_ref as MR

pytestmark = pytest.mark.gpu
P = R.P
EDGE = [0, 1, P - 1, P, 1 << 31, (1 << 32) - 1]
ROUNDS = 5


def dev(a):
    return torch.from_numpy(np.array(a, dtype=np.uint32, order="C").view(np.int32).reshape(-1)).cuda()


def host(t):
    return t.cpu().numpy().view(np.uint32)


def empty(n, fill=0):
    return torch.full((n,), fill, dtype=torch.int32, device="cuda")


def words(shape, seed):
    """random u32 words with the edge words mixed in: every fourth position cycles through EDGE"""
    w = np.random.default_rng(seed).integers(0, 1 << 32, shape, dtype=np.uint64).astype(np.uint32)
    flat = w.reshape(-1)
    idx = np.arange(0, flat.size, 4)
    flat[idx] = np.array(EDGE, np.uint64).astype(np.uint32)[(idx // 4 + seed) % 6]
    return w


def rand_elems(n, seed):
    return [tuple(int(v) for v in row) for row in np.random.default_rng(seed).integers(0, P, (n, 4))]


def circle_points(m, seed):
    return [R.circle_point(t) for t in rand_elems(m, seed)]


def planes(t, n, stride=0):
    """the four planes of a device vector -> (4, n) uint32"""
    h = host(t).reshape(-1)
    stride = stride or n
    return np.stack([h[e * stride: e * stride + n] for e in range(4)])


# ---- pointwise
@pytest.mark.parametrize("n", [1, 255, 256, 257, (1 << 16) + 3])
def test_pointwise_against_the_model(n):
    a, b = words((4, n), 100 + n % 7), words((4, n), 200 + n % 5)
    ra, rb = R.np_elems(a), R.np_elems(b)
    t_a, t_b = dev(a), dev(b)
    for op, exp in ((E.MUL, R.np_mul(ra, rb)), (E.SQR, R.np_mul(ra, ra)), (E.INV, R.np_inv(ra)), (E.MUL_BASE, R.np_mul_base(ra, rb[0]))):
        t_out = empty(4 * n, -1)
        E.pointwise_device(op, t_a, t_b if op in (E.MUL, E.MUL_BASE) else None, t_out, n)
        assert np.array_equal(planes(t_out, n), exp), op
    prod = R.np_mul(ra, R.np_inv(ra))[:, np.any(ra != 0, axis=0)]   # the model's own inverse is one
    assert (prod[0] == 1).all() and not prod[1:].any()


def test_pointwise_every_edge_word_in_every_coordinate():
    g = np.stack([x.reshape(-1) for x in np.meshgrid(*[np.array(EDGE, np.uint64)] * 4, indexing="ij")]).astype(np.uint32)   # 6^4 elements
    n = g.shape[1]
    b = np.roll(g, 7, axis=1)[::-1].copy()
    ra, rb = R.np_elems(g), R.np_elems(b)
    t_a, t_b, t_out = dev(g), dev(b), empty(4 * n, -1)
    assert np.array_equal(planes(E.pointwise_device(E.MUL, t_a, t_b, t_out, n), n), R.np_mul(ra, rb))
    assert np.array_equal(planes(E.pointwise_device(E.INV, t_a, None, t_out, n), n), R.np_inv(ra))
    assert not planes(t_out, n)[:, 0].any()   # the inverse of (0, 0, 0, 0) is 0; so is that of (p, p, p, p)
    assert not planes(t_out, n)[:, np.all(ra == 0, axis=0)].any()


def test_pointwise_in_place_and_with_strides():
    n, sa, sb, so = 257, 300, 260, 264
    a, b = words((4, sa), 11), words((4, sb), 12)
    ra, rb = R.np_elems(a[:, :n]), R.np_elems(b[:, :n])
    t_out = empty(4 * so, -1)
    E.pointwise_device(E.MUL, dev(a), dev(b), t_out, n, sa, sb, so)
    assert np.array_equal(planes(t_out, n, so), R.np_mul(ra, rb))
    assert (host(t_out).reshape(4, so)[:, n:] == 0xFFFFFFFF).all()   # nothing between the planes is written
    t_a = dev(a)
    E.pointwise_device(E.MUL, t_a, dev(b), t_a, n, sa, sb, sa)        # out is a
    assert np.array_equal(planes(t_a, n, sa), R.np_mul(ra, rb))
    assert np.array_equal(host(t_a).reshape(4, sa)[:, n:], a[:, n:])
    t_b = dev(b)
    E.pointwise_device(E.MUL, dev(a), t_b, t_b, n, sa, sb, sb)        # out is b
    assert np.array_equal(planes(t_b, n, sb), R.np_mul(ra, rb))
    t_a = dev(a)
    E.pointwise_device(E.INV, t_a, None, t_a, n, sa, 0, sa)
    assert np.array_equal(planes(t_a, n, sa), R.np_inv(ra))


def test_pointwise_inverse_where_the_norm_has_a_zero_coordinate_and_cm31_products():
    # A1 = 0: the norm is A0^2 = (a^2 - b^2, 2ab), with a zero coordinate for a = 0, b = 0 and a = +-b; A0 = 0 likewise
    special = [(0, 0, 0, 0), (3, 0, 0, 0), (0, 5, 0, 0), (4, 4, 0, 0), (4, P - 4, 0, 0), (0, 0, 3, 0), (0, 0, 0, 5), (0, 0, 4, 4), (1, 0, 0, 0), (0, 0, 1, 0)]
    norms = []
    for s in special:
        s0, nr = R.c_mul(s[:2], s[:2]), R.c_nonresidue(R.c_mul(s[2:], s[2:]))
        norms.append(((s0[0] - nr[0]) % P, (s0[1] - nr[1]) % P))
    assert sum(1 for nm in norms if 0 in nm) >= 6
    n = len(special)
    t = dev(R.np_of(special))
    got = R.elems_of(planes(E.pointwise_device(E.INV, t, None, empty(4 * n), n), n))
    assert got == [R.inv(s) for s in special]
    assert all(R.mul(s, g) == R.ONE for s, g in zip(special[1:], got[1:]))
    # both u-parts zero: the CM31 product, the u-part of the result zero
    m = 300
    a, b = words((4, m), 21), words((4, m), 22)
    a[2:], b[2:] = np.array([[0], [P]], np.uint32), 0
    out = planes(E.pointwise_device(E.MUL, dev(a), dev(b), empty(4 * m, -1), m), m)
    ra, rb = R.np_elems(a), R.np_elems(b)
    assert not out[2:].any()
    assert [tuple(int(x) for x in c) for c in out[:2].T] == [R.c_mul((int(x[0]), int(x[1])), (int(y[0]), int(y[1]))) for x, y in zip(ra.T, rb.T)]


# ---- evaluate
@pytest.mark.parametrize("log2n,n_cols,m,stride", [(1, 2, 1, 0), (2, 1, 2, 0), (3, 3, 4, 12), (10, 1, 2, 0), (11, 2, 3, 0), (12, 1, 1, 5000), (16, 2, 1, 0),
                                                   (16, 1, 4, 0), (16, 1, 5, 0)])
def test_evaluate_against_the_model(log2n, n_cols, m, stride):
    n = 1 << log2n
    s = stride or n
    cols = words((n_cols, s), 300 + log2n + m)
    pts = circle_points(m - 1, 31 + log2n) + [(rand_elems(1, 32)[0], rand_elems(1, 33)[0])]   # the last one off the circle
    got = E.evaluate_device(dev(cols), n_cols, log2n, pts, col_stride=stride)
    assert got.shape == (n_cols, m, 4) and got.dtype == np.uint32
    for k in range(n_cols):
        for j in range(m):
            assert tuple(int(x) for x in got[k, j]) == R.np_evaluate(cols[k, :n], pts[j]), (k, j)


def test_evaluate_point_words_at_the_edges_and_ext_columns():
    log2n, n = 5, 32
    cols = words((4, n), 41)
    pt_words = ((EDGE[3], EDGE[5], EDGE[4], 7), (EDGE[2], EDGE[4], EDGE[5], EDGE[3]))   # any u32 is a word of a point
    pt = (R.elem(pt_words[0]), R.elem(pt_words[1]))
    got = E.evaluate_device(dev(cols), 4, log2n, [pt_words])
    exp = [R.evaluate(cols[k].tolist(), pt) for k in range(4)]
    assert [tuple(int(x) for x in got[k, 0]) for k in range(4)] == exp
    assert E.evaluate_ext_device(dev(cols), log2n, [pt_words]) == [R.combine_planes(exp)] == [E.combine_planes(exp)]


def test_evaluate_at_a_base_field_point_is_the_transforms_value():
    log2n, n = 12, 1 << 12
    col = words((n,), 51)
    ev = circle.evaluate_cfft(col)
    pts = CR.coset_points(log2n)
    idx = [0, 1, n // 2 - 1, n - 1, 1234]
    got = E.evaluate_device(dev(col), 1, log2n, [(R.embed(pts[i][0]), R.embed(pts[i][1])) for i in idx])
    assert [tuple(int(x) for x in got[0, j]) for j in range(len(idx))] == [(int(ev[i]), 0, 0, 0) for i in idx]


# ---- DEEP quotients
def deep_case(log2n, n_cols, m, seed, stride=0, out_stride=0, zero_weight=False):
    n = 1 << log2n
    s = stride or n
    cols = words((n_cols, s), seed)
    pts = circle_points(m, seed + 1)
    ws = [rand_elems(m, seed + 2 + k) for k in range(n_cols)]
    es = [rand_elems(m, seed + 50 + k) for k in range(n_cols)]
    if zero_weight:
        ws[0][0] = R.ZERO
        ws[-1][-1] = (P, 0, P, 0)   # zero, spelled with p
    so = out_stride or n
    t_out = empty(4 * so, -1)
    E.deep_quotients_device(dev(cols), n_cols, log2n, pts, ws, es, t_out, col_stride=stride, out_stride=out_stride)
    exp = R.np_deep_quotients(cols[:, :n], log2n, pts, ws, es)
    assert np.array_equal(planes(t_out, n, so), exp)
    if so > n:
        assert (host(t_out).reshape(4, so)[:, n:] == 0xFFFFFFFF).all()


@pytest.mark.parametrize("log2n,n_cols,m", [(1, 1, 1), (2, 9, 4), (3, 1, 5), (10, 9, 1), (10, 1, 4), (10, 2, 5), (12, 9, 5), (11, 3, 2), (11, 4, 3)])
def test_deep_quotients_against_the_model(log2n, n_cols, m):
    deep_case(log2n, n_cols, m, 600 + 10 * log2n + m)


def test_deep_quotients_strides_and_a_zero_weight():
    deep_case(10, 3, 5, 71, stride=1028, out_stride=1032, zero_weight=True)
    deep_case(3, 2, 2, 72, stride=12, out_stride=8, zero_weight=True)


def test_deep_quotients_numpy_model_is_the_integer_model():
    cols = words((2, 8), 73)
    pts, ws, es = circle_points(2, 74), [rand_elems(2, 75), rand_elems(2, 76)], [rand_elems(2, 77), rand_elems(2, 78)]
    assert R.elems_of(R.np_deep_quotients(cols, 3, pts, ws, es)) == R.deep_quotients(cols.tolist(), 3, pts, ws, es)


def test_deep_quotient_is_of_low_degree_exactly_for_the_true_value():
    """n = 2^8 coefficients on N = 2^10: with v the value at P every coefficient k >= n of every plane of the quotient is
    zero; with v off by one it is not.  An Fp4 column goes in as its four planes under plane_weights."""
    lg, lgN = 8, 10
    n, N = 1 << lg, 1 << lgN
    coeffs = np.zeros((5, N), np.uint32)
    coeffs[:, :n] = words((5, n), 81)              # one base column, then the four planes of an Fp4 column
    t_coeffs = dev(coeffs)
    t_lde = empty(5 * N)
    circle.evaluate_cfft_device(t_coeffs, t_lde, lgN, batch=5)
    pts = circle_points(2, 82)
    v = E.evaluate_device(t_coeffs, 5, lg, pts, col_stride=N)
    assert tuple(int(x) for x in v[0, 0]) == R.np_evaluate(coeffs[0, :n], pts[0])
    w_base, w_ext = rand_elems(2, 83), rand_elems(2, 84)
    weights = [w_base] + E.plane_weights(w_ext)
    assert weights[1:] == R.plane_weights(w_ext)
    for off, low in ((0, True), (1, False)):
        evals = [[tuple((int(x) + (off if e == 0 else 0)) % P for e, x in enumerate(v[k, j])) for j in range(2)] for k in range(5)]
        t_q = empty(4 * N)
        E.deep_quotients_device(t_lde, 5, lgN, pts, weights, evals, t_q)
        t_c = empty(4 * N)
        circle.interpolate_cfft_device(t_q, t_c, lgN, batch=4)
        high = planes(t_c, N)[:, n:]
        assert (not high.any()) == low, off
    # the four planes as one column of Fp4 values: the same quotient as a single column whose value is the combined one
    ext_val = [R.combine_planes([tuple(int(x) for x in v[1 + e, j]) for e in range(4)]) for j in range(2)]
    assert ext_val == E.evaluate_ext_device(t_coeffs[N:], lg, pts, plane_stride=N)


# ---- fold and layers
@pytest.mark.parametrize("log2m", [1, 2, 3, 10, 16])
def test_fold_first_and_later_against_the_model(log2m):
    M = 1 << log2m
    v = words((4, M), 900 + log2m)
    zeta = rand_elems(1, 901)[0]
    for first in (True, False):
        t_out = E.fri_fold_device(dev(v), log2m, zeta, first)
        assert np.array_equal(planes(t_out, M // 2), R.np_fold(R.np_elems(v), zeta, first)), first
    if log2m <= 3:
        assert R.elems_of(R.np_fold(R.np_elems(v), zeta, True)) == R.fold(R.elems_of(R.np_elems(v)), zeta, True)
        assert R.elems_of(R.np_fold(R.np_elems(v), zeta, False)) == R.fold(R.elems_of(R.np_elems(v)), zeta, False)


def test_fold_with_strides_and_edge_words_in_zeta():
    log2m, M, si, so = 10, 1 << 10, 1040, 520
    v = words((4, si), 911)
    zeta_words = (EDGE[5], EDGE[3], EDGE[4], EDGE[2])
    t_out = empty(4 * so, -1)
    E.fri_fold_device(dev(v), log2m, zeta_words, False, t_out, in_stride=si, out_stride=so)
    assert np.array_equal(planes(t_out, M // 2, so), R.np_fold(R.np_elems(v[:, :M]), R.elem(zeta_words), False))
    assert (host(t_out).reshape(4, so)[:, M // 2:] == 0xFFFFFFFF).all()


@pytest.mark.parametrize("log2m,first", [(3, True), (3, False), (4, True), (10, False), (16, True)])
def test_layer_root_is_the_commitment_of_the_pair_columns(log2m, first):
    M = 1 << log2m
    v = words((4, M), 920 + log2m)
    zeta = rand_elems(1, 921)[0]
    t_folded, t_nodes, root = E.fri_layer_device(dev(v), log2m, zeta, first, ROUNDS)
    folded = R.np_fold(R.np_elems(v), zeta, first)
    assert np.array_equal(planes(t_folded, M // 2), folded)
    pair_cols = R.np_pair_columns(folded)
    assert pair_cols.shape == (8, M // 4)
    exp_root, exp_nodes = monolith.commit_columns(ROUNDS, pair_cols, bit_reverse=False, return_nodes=True)
    assert np.array_equal(root, exp_root)
    assert np.array_equal(host(t_nodes).reshape(-1, 8), exp_nodes)
    if log2m <= 10:
        assert np.array_equal(exp_nodes, MR.np_tree(ROUNDS, pair_cols, False))


@pytest.mark.parametrize("log2m", [3, 4, 10, 16])
def test_layer_writes_its_pair_columns_and_nodes_and_nothing_around_them(log2m):
    """The C entry on buffers with guard words on both sides: the eight pair columns are 2 M words, the nodes M / 2 - 1 digests."""
    from lambda_elliptic_curves_amd import _lib as L
    from lambda_elliptic_curves_amd.errors import check
    M, G = 1 << log2m, 64
    half = M // 2
    v = words((4, M), 960 + log2m)
    zeta = np.array(rand_elems(1, 961)[0], np.uint32)
    t_v, t_out, t_pairs, t_nodes = dev(v), empty(4 * half + 2 * G, -1), empty(4 * half + 2 * G, -1), empty(8 * (half - 1) + 2 * G, -1)
    root = np.zeros(8, np.uint32)
    check(L.lib().lw_mersenne31_ext4_fri_layer_device(L.device_ptr(t_v), 0, log2m, L.host_ptr(zeta), 0, L.device_ptr(t_out[G:]), 0, ROUNDS,
                                                     L.device_ptr(t_pairs[G:]), L.device_ptr(t_nodes[G:]), L.host_ptr(root), L.stream_ptr(None)))
    folded = R.np_fold(R.np_elems(v), tuple(int(z) for z in zeta), False)
    pair_cols = R.np_pair_columns(folded)
    for t, body in ((t_out, folded.reshape(-1)), (t_pairs, pair_cols.reshape(-1))):
        h = host(t)
        assert (h[:G] == 0xFFFFFFFF).all() and (h[-G:] == 0xFFFFFFFF).all()
        assert np.array_equal(h[G:-G], body)
    h = host(t_nodes)
    assert (h[:G] == 0xFFFFFFFF).all() and (h[-G:] == 0xFFFFFFFF).all()
    exp_root, exp_nodes = monolith.commit_columns(ROUNDS, pair_cols, bit_reverse=False, return_nodes=True)
    assert np.array_equal(h[G:-G].reshape(-1, 8), exp_nodes) and np.array_equal(root, exp_root)


def transcript(prev):
    """zeta from the root of the layer before (None: a fixed seed), through the hash of the trees"""
    seed = [0] * 8 if prev is None else [int(x) for x in prev]
    return tuple(MR.hash(ROUNDS, seed + [7])[:4])


def model_commit_phase(v, number_layers):
    layers, prev = [], None
    for k in range(number_layers):
        v = R.np_fold(v, transcript(prev), k == 0)
        if k + 1 < number_layers:
            nodes = MR.np_tree(ROUNDS, R.np_pair_columns(v), False)
            layers.append((v, nodes))
            prev = nodes[0]
    return v, layers


def test_commit_phase_from_2_to_the_12_and_one_opening_per_layer():
    log2n, N, number_layers = 12, 1 << 12, 10
    v = words((4, N), 931)
    last, layers = E.fri_commit_phase_device(dev(v), log2n, number_layers, ROUNDS, transcript)
    exp_last, exp_layers = model_commit_phase(R.np_elems(v), number_layers)
    assert last == R.elems_of(exp_last) and len(last) == N >> number_layers
    assert len(layers) == number_layers - 1 == len(exp_layers)
    trees, positions = [], []
    for k, ((t_ev, t_nodes, root), (ev, nodes)) in enumerate(zip(layers, exp_layers)):
        M = N >> (k + 1)
        assert np.array_equal(planes(t_ev, M), ev) and np.array_equal(host(t_nodes).reshape(-1, 8), nodes) and np.array_equal(root, nodes[0])
        trees.append(merkle.Tree(fft.Stark252PrimeField, t_nodes, log2n - k - 2))   # 32-byte nodes, root first, no columns
        positions.append((5 * k + 3) % (M // 2))
    assert layers[-1][0].numel() == 4 * 8   # the smallest committed layer: 8 values, 4 leaves
    # every tree at its own leaf, one gather
    _, paths = merkle.open_trees_device(trees, np.array([[p] for p in positions], np.uint64))
    for k, (ev, nodes) in enumerate(exp_layers):
        leaves, pos = ev.shape[1] // 2, positions[k]
        cur = MR.hash(ROUNDS, [int(x) for x in R.np_pair_columns(ev)[:, pos]])
        assert cur == nodes[leaves - 1 + pos].tolist()
        i = pos
        for sib in paths[k][0].view(np.uint32).reshape(-1, 8).tolist():
            cur = MR.compress(ROUNDS, cur, sib) if i % 2 == 0 else MR.compress(ROUNDS, sib, cur)
            i >>= 1
        assert cur == nodes[0].tolist(), k


def test_commit_phase_refuses_layers_it_cannot_commit_or_fold():
    from lambda_elliptic_curves_amd import errors
    t = dev(words((4, 16), 941))
    for bad in (0, 5, 4):   # 4 folds of 16 values would commit a layer of 2
        with pytest.raises(errors.InputError):
            E.fri_commit_phase_device(t, 4, bad, ROUNDS, transcript)
    last, layers = E.fri_commit_phase_device(t, 4, 3, ROUNDS, transcript)
    assert len(last) == 2 and [x[0].numel() for x in layers] == [32, 16]
    last, layers = E.fri_commit_phase_device(t, 4, 1, ROUNDS, transcript)
    assert len(last) == 8 and layers == []


# ---- the chain
def test_chain_from_the_lde_to_a_constant_last_layer():
    """circle.lde_device -> monolith.commit_columns_device -> interpolate -> evaluate -> deep_quotients -> commit phase at
    trace 2^8, blow-up 4: every step reads the tensor the step before left on the device."""
    lg, lgN, n_cols = 8, 10, 3
    n, N = 1 << lg, 1 << lgN
    trace = words((n_cols, n), 951)
    t_lde = empty(n_cols * N)
    circle.lde_device(dev(trace), lg, t_lde, lgN, batch=n_cols)
    t_nodes = torch.empty((2 * N - 1, 8), dtype=torch.int32, device="cuda")
    root = monolith.commit_columns_device(ROUNDS, t_lde, n_cols, lgN, t_nodes)
    t_coeffs = empty(n_cols * N)
    circle.interpolate_cfft_device(t_lde, t_coeffs, lgN, batch=n_cols)
    pts = circle_points(2, 952)
    v = E.evaluate_device(t_coeffs, n_cols, lg, pts, col_stride=N)
    evals = [[tuple(int(x) for x in v[k, j]) for j in range(2)] for k in range(n_cols)]
    weights = [rand_elems(2, 953 + k) for k in range(n_cols)]
    t_deep = empty(4 * N)
    E.deep_quotients_device(t_lde, n_cols, lgN, pts, weights, evals, t_deep)
    last, layers = E.fri_commit_phase_device(t_deep, lgN, lg, ROUNDS, transcript)
    # the model, from the trace
    lde = CR.np_lde(trace, lgN)
    assert np.array_equal(host(t_lde).reshape(n_cols, N), lde)
    assert np.array_equal(root, MR.np_tree(ROUNDS, lde, True)[0])
    coeffs = CR.np_interpolate_cfft(trace)
    assert evals == [[R.np_evaluate(coeffs[k], pt) for pt in pts] for k in range(n_cols)]
    deep = R.np_deep_quotients(lde, lgN, pts, weights, evals)
    assert np.array_equal(planes(t_deep, N), deep)
    exp_last, exp_layers = model_commit_phase(deep, lg)
    assert last == R.elems_of(exp_last) and len(last) == 4
    assert last[0] == last[1] == last[2] == last[3] and last[0] != R.ZERO   # degree below 2^8: constant after 8 folds
    assert [np.array_equal(r, nodes[0]) for (_, _, r), (_, nodes) in zip(layers, exp_layers)] == [True] * (lg - 1)
