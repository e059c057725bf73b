"""The quartic extension of Mersenne31 without a device: the model the GPU tests compare against (tests/mersenne31_ext_ref.py)
pinned by the reference's own unit-test values and by the properties the prover steps rest on, the arithmetic header and the
host tables compiled for the host and run under sanitizers against that model, and the argument checks of the new entry
points, which all run before any device work."""
import ctypes as C
import json
import os
import random
import subprocess

import numpy as np
import pytest

from tests import circle_ref as CR
from tests import mersenne31_ext_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = R.P
EDGE = [0, 1, P - 1, P, 1 << 31, (1 << 32) - 1]
SYMBOLS = ["lw_mersenne31_ext4_pointwise_device", "lw_mersenne31_ext4_evaluate_device", "lw_mersenne31_ext4_deep_quotients_device",
           "lw_mersenne31_ext4_fri_layer_device"]


def rand_elems(n, seed):
    rnd = random.Random(seed)
    return [tuple(rnd.randrange(P) for _ in range(4)) for _ in range(n)]


def evaluations(coeffs):
    """the values of a polynomial with QM31 coefficients on the standard coset, plane by plane"""
    planes = [CR.evaluate_cfft([c[e] for c in coeffs]) for e in range(4)]
    return [tuple(planes[e][i] for e in range(4)) for i in range(len(coeffs))]


# ---- the model
def test_model_reproduces_the_values_of_the_references_unit_tests():
    kat = json.load(open(os.path.join(ROOT, "tests", "golden", "mersenne31_ext_kat.json")))
    assert kat["p"] == P
    red = lambda v: tuple(x % P for x in v)
    for t in kat["fp2_mul"]:
        assert R.c_mul(red(t["a"]), red(t["b"])) == red(t["c"]), t["name"]
        assert R.mul(red(t["a"]) + (0, 0), red(t["b"]) + (0, 0)) == red(t["c"]) + (0, 0), t["name"]
    for t in kat["fp2_inv"]:
        assert R.c_inv(red(t["a"])) == red(t["c"]), t["name"]
        assert R.inv(red(t["a"]) + (0, 0)) == red(t["c"]) + (0, 0), t["name"]
    for a in kat["fp2_mul_inv_is_one"]:
        assert R.c_mul(red(a), R.c_inv(red(a))) == (1, 0)
    for t in kat["fp2_div"]:
        assert R.c_mul(red(t["a"]), R.c_inv(red(t["b"]))) == red(t["c"]), t["name"]
    for a in kat["fp2_square_equals_mul"]:
        assert R.sqr(red(a) + (0, 0)) == R.c_mul(red(a), red(a)) + (0, 0)
    for a in kat["fp4_mul_by_zero_and_one"]:
        assert R.mul(red(a), R.ZERO) == R.ZERO and R.mul(red(a), R.ONE) == red(a)
    for a in kat["fp4_square_equals_mul"]:
        assert R.sqr(red(a)) == R.mul(red(a), red(a))
    for a in kat["fp4_mul_by_inv_is_one"]:
        assert R.mul(red(a), R.inv(red(a))) == R.ONE
    mb = kat["fp4_mul_base"]
    assert R.mul_base(red(mb["b"]), mb["a"] % P) == R.mul(R.embed(mb["a"]), red(mb["b"]))


def test_model_field_has_inverses_and_the_nonresidue_rule():
    edge = [R.elem((a, b, c, d)) for a in EDGE for b in EDGE[:3] for c in EDGE[1:4] for d in EDGE[2:]]
    for a in edge + rand_elems(500, 1):
        if a != R.ZERO:
            assert R.mul(a, R.inv(a)) == R.ONE, a
        assert R.sqr(a) == R.mul(a, a)
    assert R.inv(R.ZERO) == R.ZERO
    u, i = (0, 0, 1, 0), (0, 1, 0, 0)
    assert R.mul(u, u) == (2, 1, 0, 0) and R.mul(i, i) == (P - 1, 0, 0, 0)          # u^2 = 2 + i, i^2 = -1
    assert R.c_nonresidue((5, 7)) == R.c_mul((2, 1), (5, 7))                        # (a, b) -> (2a - b, 2b + a)
    a, b = rand_elems(2, 2)
    assert R.conj(R.mul(a, b)) == R.mul(R.conj(a), R.conj(b)) and R.conj(R.embed(9)) == R.embed(9)
    assert R.times_u(a) == R.mul(a, u) and R.times_i(a) == R.mul(a, i)
    assert R.combine_planes([a, b, a, b]) == R.add(R.add(a, R.mul(i, b)), R.add(R.mul(u, a), R.mul(R.mul(i, u), b)))
    # the numpy forms are the integer forms
    A, B = rand_elems(40, 3) + [R.ZERO, (0, 0, 5, 7), (3, 0, 0, 0)], rand_elems(43, 4)
    assert R.elems_of(R.np_mul(R.np_of(A), R.np_of(B))) == [R.mul(x, y) for x, y in zip(A, B)]
    assert R.elems_of(R.np_inv(R.np_of(A))) == [R.inv(x) for x in A]


def test_model_point_lies_on_the_circle_and_the_line_vanishes_at_it():
    X, Y = R.circle_point(rand_elems(1, 5)[0])
    assert R.add(R.sqr(X), R.sqr(Y)) == R.ONE
    sX, sY = R.conj(X), R.conj(Y)
    line = lambda x, y: R.add(R.add(R.mul(R.sub(Y, sY), x), R.mul(R.sub(sX, X), y)), R.sub(R.mul(X, sY), R.mul(Y, sX)))
    assert line(X, Y) == R.ZERO and line(sX, sY) == R.ZERO
    for x, y in CR.coset_points(4):
        D = line(R.embed(x), R.embed(y))
        assert D[0] == 0 and D[1] == 0 and D != R.ZERO   # u times a CM31 value, never zero on the domain


def test_model_deep_quotient_is_of_low_degree_exactly_for_the_true_value():
    n, lgN = 8, 5
    rnd = random.Random(6)
    col = [rnd.randrange(1 << 32) for _ in range(n)]
    ev = CR.evaluate_cfft(col + [0] * ((1 << lgN) - n))
    pt = R.circle_point(rand_elems(1, 7)[0])
    v, w = R.evaluate(col, pt), rand_elems(1, 8)[0]
    assert R.np_evaluate(col, pt) == v
    for off in (0, 1):
        q = R.deep_quotients([ev], lgN, [pt], [[w]], [[R.add(v, R.embed(off))]])
        assert R.elems_of(R.np_deep_quotients([ev], lgN, [pt], [[w]], [[R.add(v, R.embed(off))]])) == q
        for e in range(4):
            high = CR.interpolate_cfft([x[e] for x in q])[n:]
            assert any(high) == bool(off), (off, e)


def test_model_fold_of_the_evaluations_is_the_evaluation_of_the_coefficient_fold():
    c = rand_elems(32, 9)
    v = evaluations(c)
    first = True
    while len(v) > 1:
        zeta = rand_elems(1, 10 + len(v))[0]
        assert R.elems_of(R.np_fold(R.np_of(v), zeta, first)) == R.fold(v, zeta, first)
        v, c = R.fold(v, zeta, first), R.fold_coeffs(c, zeta)
        # the layer lives on the x of the first M points of the coset of size 2M, in the basis prod pi^(j-1)(x)^(bit j of m)
        xs = [q[0] for q in CR.coset_points(len(v).bit_length())[: len(v)]]
        exp = []
        for x in xs:
            total = R.ZERO
            for m, cm in enumerate(c):
                total = R.add(total, R.mul_base(cm, CR.basis_value(2 * m, x, 0)))
            exp.append(total)
        assert v == exp, len(v)
        first = False
    assert len(c) == 1 and v == c


def test_model_layer_tree_and_commit_phase():
    from tests import monolith_ref as MR
    v = rand_elems(16, 11)
    cols = R.pair_columns(v)
    assert len(cols) == 8 and all(len(col) == 8 for col in cols) and R.np_pair_columns(R.np_of(v)).tolist() == cols
    nodes = R.layer_tree(5, v)
    assert nodes.shape == (15, 8)
    assert nodes[7 + 3].tolist() == MR.hash(5, list(v[3]) + list(v[12]))
    assert nodes[0].tolist() == MR.compress(5, nodes[1].tolist(), nodes[2].tolist())
    seen = []

    def challenge(prev):
        seen.append(None if prev is None else [int(x) for x in prev])
        return (len(seen), 2, 3, 4)
    last, layers = R.commit_phase(v, 3, 5, challenge)
    assert len(last) == 2 and [len(lv) for lv, _ in layers] == [8, 4] and seen == [None] + [nd[0].tolist() for _, nd in layers]
    assert layers[0][0] == R.fold(v, (1, 2, 3, 4), True) and last == R.fold(layers[1][0], (3, 2, 3, 4), False)


# ---- the arithmetic header and the host tables, sanitised, as a child process
def test_host_program_of_the_arithmetic_and_the_tables(tmp_path):
    hipcc = "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        hipcc = "hipcc"
    exe = tmp_path / "mersenne31_ext_host"
    subprocess.check_call([hipcc, "-x", "hip", "--cuda-host-only", "-O2", "-std=c++17", "-Xarch_host", "-fsanitize=address,undefined",
                           "-Xarch_host", "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "lambda_elliptic_curves_amd", "csrc"),
                           os.path.join(ROOT, "tests", "mersenne31_ext_host_main.cpp"), "-o", str(exe)], timeout=600)
    n_cols, m, log2n = 3, 5, 7
    rnd = random.Random(12)
    word = lambda k: EDGE[k % 6] if k % 3 == 0 else rnd.randrange(1 << 32)
    points = [word(k) for k in range(8 * m)]
    weights = [word(k + 1) for k in range(4 * n_cols * m)]
    evals = [word(k + 2) for k in range(4 * n_cols * m)]
    out = subprocess.run([str(exe), str(len(EDGE))] + [str(v) for v in EDGE + [n_cols, m, log2n] + points + weights + evals], capture_output=True, text=True,
                         timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    got = [tuple(int(x) for x in line.split()) for line in out.stdout.splitlines()]
    at = 0

    def take(k):
        nonlocal at
        at += k
        return got[at - k: at]
    ea = [R.elem((a, b, c, d)) for a in EDGE for b in EDGE for c in EDGE for d in EDGE]
    ne = len(ea)
    assert take(ne) == [R.mul(a, ea[(7 * i + 3) % ne]) for i, a in enumerate(ea)]
    assert take(3 * ne) == [r for a in ea for r in (R.sqr(a), R.inv(a), R.mul(a, R.inv(a)))]
    assert take(6 * ne) == [R.mul_base(a, CR.reduce_word(b)) for a in ea for b in EDGE]
    pts = [(R.elem(points[8 * j: 8 * j + 4]), R.elem(points[8 * j + 4: 8 * j + 8])) for j in range(m)]
    W = [[R.elem(weights[4 * (k * m + j): 4 * (k * m + j) + 4]) for j in range(m)] for k in range(n_cols)]
    V = [[R.elem(evals[4 * (k * m + j): 4 * (k * m + j) + 4]) for j in range(m)] for k in range(n_cols)]
    for X, Y in pts:
        assert take(8) == [R.basis_value(e, X, Y) for e in range(8)]
        f = [Y, X]
        while len(f) < 30:
            f.append(R.sub(R.mul_base(R.sqr(f[-1]), 2), R.ONE))
        assert take(30) == f
    uinv = R.inv((0, 0, 1, 0))
    cc = []
    for j, (X, Y) in enumerate(pts):
        X0, X1, Y0, Y1 = X[:2], X[2:], Y[:2], Y[2:]
        dbl = lambda a: (2 * a[0] % P, 2 * a[1] % P)
        neg = lambda a: (-a[0] % P, -a[1] % P)
        t, s = R.c_mul(X1, Y0), R.c_mul(X0, Y1)
        cc.append(neg(dbl(Y1)))
        assert take(2) == [dbl(Y1) + neg(dbl(X1)), dbl(((t[0] - s[0]) % P, (t[1] - s[1]) % P)) + cc[-1]]
        # D = u d: the constants are those of the line
        D = lambda x, y: R.add(R.add(R.mul_base(R.sub(Y, R.conj(Y)), x), R.mul_base(R.sub(R.conj(X), X), y)), R.sub(R.mul(X, R.conj(Y)), R.mul(Y, R.conj(X))))
        da, db, dc = got[at - 2][:2], got[at - 2][2:], got[at - 1][:2]
        for x, y in ((3, 5), (P - 1, 77)):
            d = tuple((da[e] * x + db[e] * y + dc[e]) % P for e in range(2))
            assert R.times_u(d + (0, 0)) == D(x, y)
        cj = R.sub(R.conj(Y), Y)
        sa = sb = R.ZERO
        for k in range(n_cols):
            a = R.sub(R.conj(V[k][j]), V[k][j])
            sa = R.add(sa, R.mul(W[k][j], a))
            sb = R.add(sb, R.mul(W[k][j], R.sub(R.mul(V[k][j], cj), R.mul(a, Y))))
        assert take(2) == [R.mul(sa, uinv), R.mul(sb, uinv)]
    groups = (m + 3) // 4
    exp = [[[R.ZERO] * 4 for _ in range(n_cols)] for _ in range(groups)]
    for k in range(n_cols):
        for j in range(m):
            exp[j // 4][k][j % 4] = R.mul(W[k][j], cc[j] + (0, 0))
    assert take(groups * n_cols * 4) == [w for g in exp for row in g for w in row]
    shift, step = CR.subgroup_generator(log2n + 1), CR.subgroup_generator(log2n)
    assert take(1) == [shift + (0, 0)]
    assert take(30) == [(CR.pmul(1 << b, step) if b < log2n else (1, 0)) + (0, 0) for b in range(30)]
    assert at == len(got)


# ---- the boundary
def test_symbols_are_exported_and_declared():
    from lambda_elliptic_curves_amd import _lib
    L = _lib.lib()
    header = open(os.path.join(ROOT, "include", "lw_hip.h")).read()
    ffi = open(os.path.join(ROOT, "rust-shim", "src", "ffi.rs")).read()
    for sym in SYMBOLS:
        assert sym in _lib.EXPORTS and hasattr(L, sym)
        assert "int %s(" % sym in header and "pub fn %s(" % sym in ffi
    for k, name in enumerate(("MUL", "SQR", "INV", "MUL_BASE")):
        assert "LW_M31EXT4_%s = %d" % (name, k) in header and "pub const LW_M31EXT4_%s: c_int = %d;" % (name, k) in ffi
        assert getattr(_lib, "M31EXT4_" + name) == k


def test_python_helpers_are_the_models():
    from lambda_elliptic_curves_amd import mersenne31_ext as E
    a, b = rand_elems(2, 13)
    assert E.P == P and E.times_i(a) == R.times_i(a) and E.times_u(a) == R.times_u(a)
    assert E.combine_planes([a, b, b, a]) == R.combine_planes([a, b, b, a])
    assert E.plane_weights([a, b]) == R.plane_weights([a, b])
    assert E.times_u((P, 1 << 31, (1 << 32) - 1, 0)) == R.times_u(R.elem((P, 1 << 31, (1 << 32) - 1, 0)))
    assert E._points([(a, b)]).tolist() == [list(a) + list(b)] and E._scalars([EDGE[2:]], 1).tolist() == [EDGE[2:]]


def test_commit_phase_refuses_a_number_of_layers_before_any_device_work():
    from lambda_elliptic_curves_amd import errors
    from lambda_elliptic_curves_amd import mersenne31_ext as E

    def never(prev):
        raise AssertionError("the transcript is not asked before the layers are checked")
    for log2n, layers in ((4, 0), (4, 5), (4, 4), (1, 2), (0, 1), (31, 3), (12, 12)):
        with pytest.raises(errors.InputError):
            E.fri_commit_phase_device(None, log2n, layers, 5, never)


def test_status_codes_need_no_device():
    from lambda_elliptic_curves_amd import _lib
    L = C.CDLL(_lib.LIB_PATH)   # a handle of its own: plain ctypes arguments, no argtypes
    raw = np.zeros((1 << 13) + 4, np.uint32)
    base = (raw.ctypes.data + 15) & ~15
    at = lambda w: C.c_void_p(base + 4 * w)
    A, B, O, N = at(0), at(2048), at(4096), C.c_void_p(None)
    u32, sz, i = C.c_uint32, C.c_size_t, C.c_int
    BAD, ORDER = _lib.ERR_BAD_ARG, _lib.ERR_ORDER_TOO_LARGE
    pts = (C.c_uint32 * 16)(1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 0, 0, 11, 12, 0, 0)   # the second point is its own conjugate
    pts_p = (C.c_uint32 * 8)(1, 2, P, P, 5, 6, 0, P)                          # ... and so is this one, its zeros spelled p
    tab = (C.c_uint32 * 64)(*range(64))
    vals = (C.c_uint32 * 16)(*([99] * 16))
    pw = lambda op, a, sa, b, sb, o, so, n: L.lw_mersenne31_ext4_pointwise_device(i(op), a, sz(sa), b, sz(sb), o, sz(so), sz(n), N)
    ev = lambda c, k, s, lg, p, m, v: L.lw_mersenne31_ext4_evaluate_device(c, u32(k), sz(s), u32(lg), p, u32(m), v, N)
    dq = lambda c, k, s, lg, p, m, w, e, o, so: L.lw_mersenne31_ext4_deep_quotients_device(c, u32(k), sz(s), u32(lg), p, u32(m), w, e, o, sz(so), N)
    fl = lambda v, s, lg, z, first, o, so, r, pr, nd, rt: L.lw_mersenne31_ext4_fri_layer_device(v, sz(s), u32(lg), z, i(first), o, sz(so), u32(r), pr, nd, rt, N)
    cases = [
        ("pointwise op", lambda: pw(4, A, 0, B, 0, O, 0, 8), BAD),
        ("pointwise null a", lambda: pw(0, N, 0, B, 0, O, 0, 8), BAD),
        ("pointwise null b for mul", lambda: pw(0, A, 0, N, 0, O, 0, 8), BAD),
        ("pointwise null b for mul_base", lambda: pw(3, A, 0, N, 0, O, 0, 8), BAD),
        ("pointwise null out", lambda: pw(1, A, 0, N, 0, N, 0, 8), BAD),
        ("pointwise misaligned", lambda: pw(1, at(1), 0, N, 0, O, 0, 8), BAD),
        ("pointwise a stride", lambda: pw(1, A, 7, N, 0, O, 0, 8), BAD),
        ("pointwise out stride", lambda: pw(1, A, 0, N, 0, O, 7, 8), BAD),
        ("pointwise b stride", lambda: pw(0, A, 0, B, 7, O, 0, 8), BAD),
        ("pointwise out overlaps a", lambda: pw(1, A, 0, N, 0, at(4), 0, 8), BAD),
        ("pointwise out is a under another stride", lambda: pw(1, A, 8, N, 0, A, 12, 8), BAD),
        ("pointwise n = 0", lambda: pw(0, N, 0, N, 0, N, 0, 0), _lib.OK),
        ("evaluate log2n 0", lambda: ev(A, 1, 0, 0, pts, 1, vals), BAD),
        ("evaluate log2n 31", lambda: ev(A, 1, 0, 31, pts, 1, vals), ORDER),
        ("evaluate null points", lambda: ev(A, 1, 0, 3, N, 1, vals), BAD),
        ("evaluate null values", lambda: ev(A, 1, 0, 3, pts, 1, N), BAD),
        ("evaluate null coefficients", lambda: ev(N, 1, 0, 3, pts, 1, vals), BAD),
        ("evaluate misaligned", lambda: ev(at(2), 1, 0, 3, pts, 1, vals), BAD),
        ("evaluate stride", lambda: ev(A, 2, 7, 3, pts, 1, vals), BAD),
        ("evaluate no columns", lambda: ev(N, 0, 0, 3, pts, 1, vals), _lib.OK),
        ("deep log2n 0", lambda: dq(A, 1, 0, 0, pts, 1, tab, tab, O, 0), BAD),
        ("deep log2n 31", lambda: dq(A, 1, 0, 31, pts, 1, tab, tab, O, 0), ORDER),
        ("deep no columns", lambda: dq(A, 0, 0, 3, pts, 1, tab, tab, O, 0), BAD),
        ("deep no points", lambda: dq(A, 1, 0, 3, pts, 0, tab, tab, O, 0), BAD),
        ("deep null points", lambda: dq(A, 1, 0, 3, N, 1, tab, tab, O, 0), BAD),
        ("deep null weights", lambda: dq(A, 1, 0, 3, pts, 1, N, tab, O, 0), BAD),
        ("deep null evals", lambda: dq(A, 1, 0, 3, pts, 1, tab, N, O, 0), BAD),
        ("deep null columns", lambda: dq(N, 1, 0, 3, pts, 1, tab, tab, O, 0), BAD),
        ("deep null out", lambda: dq(A, 1, 0, 3, pts, 1, tab, tab, N, 0), BAD),
        ("deep column stride", lambda: dq(A, 2, 7, 3, pts, 1, tab, tab, O, 0), BAD),
        ("deep out stride", lambda: dq(A, 1, 0, 3, pts, 1, tab, tab, O, 7), BAD),
        ("deep out overlaps the columns", lambda: dq(A, 2, 0, 3, pts, 1, tab, tab, at(8), 0), BAD),
        ("deep point is its own conjugate", lambda: dq(A, 1, 0, 3, pts, 2, tab, tab, O, 0), BAD),
        ("deep point is its own conjugate, zeros as p", lambda: dq(A, 1, 0, 3, pts_p, 1, tab, tab, O, 0), BAD),
        ("fold log2m 0", lambda: fl(A, 0, 0, tab, 1, O, 0, 0, N, N, N), BAD),
        ("fold log2m 31", lambda: fl(A, 0, 31, tab, 1, O, 0, 0, N, N, N), ORDER),
        ("later fold log2m 30", lambda: fl(A, 0, 30, tab, 0, O, 0, 0, N, N, N), ORDER),
        ("fold null zeta", lambda: fl(A, 0, 4, N, 1, O, 0, 0, N, N, N), BAD),
        ("fold null evals", lambda: fl(N, 0, 4, tab, 1, O, 0, 0, N, N, N), BAD),
        ("fold null out", lambda: fl(A, 0, 4, tab, 1, N, 0, 0, N, N, N), BAD),
        ("fold in stride", lambda: fl(A, 15, 4, tab, 1, O, 0, 0, N, N, N), BAD),
        ("fold out stride", lambda: fl(A, 0, 4, tab, 1, O, 7, 0, N, N, N), BAD),
        ("fold in place", lambda: fl(A, 0, 4, tab, 1, A, 0, 0, N, N, N), BAD),
        ("fold out overlaps the evaluations", lambda: fl(A, 0, 4, tab, 0, at(60), 0, 0, N, N, N), BAD),
        ("fold pairs without nodes", lambda: fl(A, 0, 4, tab, 1, O, 0, 5, B, N, N), BAD),
        ("fold root without nodes", lambda: fl(A, 0, 4, tab, 1, O, 0, 5, N, N, vals), BAD),
        ("layer below 4 values", lambda: fl(A, 0, 2, tab, 1, O, 0, 5, B, at(3072), N), BAD),
        ("layer rounds 0", lambda: fl(A, 0, 4, tab, 1, O, 0, 0, B, at(3072), N), BAD),
        ("layer rounds 16", lambda: fl(A, 0, 4, tab, 1, O, 0, 16, B, at(3072), N), BAD),
        ("layer nodes without pairs", lambda: fl(A, 0, 4, tab, 1, O, 0, 5, N, at(3072), N), BAD),
        ("layer pairs overlap out", lambda: fl(A, 0, 4, tab, 1, O, 0, 5, at(4100), at(3072), N), BAD),
        ("layer nodes overlap pairs", lambda: fl(A, 0, 4, tab, 1, O, 0, 5, B, at(2052), N), BAD),
        ("layer nodes overlap the last pair column", lambda: fl(A, 0, 4, tab, 1, O, 0, 5, B, at(2048 + 28), N), BAD),   # 8 columns of 4 words
        ("layer pairs end in the evaluations", lambda: fl(at(2048 + 28), 0, 4, tab, 1, O, 0, 5, B, at(3072), N), BAD),
    ]
    got = {name: call() for name, call, _ in cases}
    assert got == {name: code for name, _, code in cases}
    assert not raw.any() and list(vals) == [99] * 16


def test_no_device_is_an_error_not_a_fallback():
    import torch
    if torch.cuda.is_available():
        return   # with a device the same calls are the GPU tests' business
    from lambda_elliptic_curves_amd import _lib
    L = C.CDLL(_lib.LIB_PATH)
    raw = np.zeros(1 << 11, np.uint32)
    base = (raw.ctypes.data + 15) & ~15
    at = lambda w: C.c_void_p(base + 4 * w)
    N, sz, u32, i = C.c_void_p(None), C.c_size_t, C.c_uint32, C.c_int
    pts = (C.c_uint32 * 8)(1, 2, 3, 4, 5, 6, 7, 8)
    tab = (C.c_uint32 * 8)(*range(8))
    vals = (C.c_uint32 * 4)()
    assert L.lw_mersenne31_ext4_pointwise_device(i(0), at(0), sz(0), at(64), sz(0), at(128), sz(0), sz(8), N) == _lib.ERR_NO_DEVICE
    assert L.lw_mersenne31_ext4_evaluate_device(at(0), u32(1), sz(0), u32(3), pts, u32(1), vals, N) == _lib.ERR_NO_DEVICE
    assert L.lw_mersenne31_ext4_deep_quotients_device(at(0), u32(1), sz(0), u32(3), pts, u32(1), tab, tab, at(64), sz(0), N) == _lib.ERR_NO_DEVICE
    assert L.lw_mersenne31_ext4_fri_layer_device(at(0), sz(0), u32(4), tab, i(1), at(64), sz(0), u32(5), at(128), at(256), N, N) == _lib.ERR_NO_DEVICE
    assert not raw.any()
