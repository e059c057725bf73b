"""Starknet Pedersen hash without a device: the big-integer model (tests/pedersen_ref.py) against the recorded vectors
(tests/golden/pedersen_starkcurve.json), the library's generated lookup tables against the model's and the recorded
entries, the exported symbols, the argument checks of the C entry points, and a host build of the hash and the group
law (the device functions' own source) under ASan + UBSan in a stand-alone program."""
import ctypes as C
import json
import os
import subprocess
import textwrap

import numpy as np
import pytest

from tests import pedersen_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["lw_pedersen_hash", "lw_pedersen_hash_device", "lw_pedersen_commit_leaves", "lw_pedersen_commit_leaves_device",
           "lw_pedersen_table", "lw_pedersen_add_affine_device"]


def golden():
    with open(os.path.join(ROOT, "tests", "golden", "pedersen_starkcurve.json")) as f:
        return json.load(f)


def h(s):
    return int(s, 16)


def test_model_reproduces_the_golden_file():
    g = golden()
    assert len(g["hash"]) == 3 and len(g["table"]) == 12
    for c in g["hash"]:
        assert R.hash(h(c["x"]), h(c["y"])) == h(c["expected"]), c["cite"]
    assert h(g["hash"][1]["expected"]) == R.P0[0] and h(g["hash"][2]["x"]) == R.P - 1
    t = R.tables()
    offsets = {"T1": 0, "T2": R.N_LOW, "T3": R.N_LOW + R.TABLE_SIZE, "T4": 2 * R.N_LOW + R.TABLE_SIZE}
    for e in g["table"]:
        assert offsets[e["table"]] + e["entry"] == e["index"]
        assert t[e["index"]] == (h(e["x"]), h(e["y"])), (e["table"], e["entry"])


def test_model_tables_are_multiples_of_independent_bases():
    t = R.tables()
    assert all(R.on_curve(pt) for pt in t + [R.P0, R.P1, R.P2, R.P3, R.P4])
    assert t[0] == R.P1 and t[930] == R.P2 and t[945] == R.P3 and t[1875] == R.P4
    # T1[15 i] = 16 * T1[15 (i - 1)] and T1[15 i + k - 1] = T1[15 i + k - 2] + T1[15 i], by the affine law alone
    sixteen = t[0]
    for _ in range(4):
        sixteen = R.add(sixteen, sixteen)
    assert t[15] == sixteen and t[16] == R.add(t[15], t[15]) and t[929] == R.add(t[928], t[915])
    # P2 is not 2^248 P1: the bases are independent
    top = t[915]   # 2^244 P1
    for _ in range(4):
        top = R.add(top, top)
    assert top != R.P2


def test_model_group_law_cases():
    q = R.P1
    assert R.add(None, q) == q and R.add(q, None) == q and R.add(q, R.neg(q)) is None
    assert R._jac_add_affine((1, 1, 0), q) == (q[0], q[1], 1)
    for z in (1, 2, R.P - 1, 0x1234567):
        acc = (q[0] * z * z % R.P, q[1] * z ** 3 % R.P, z)
        d = R._jac_add_affine(acc, q)
        assert (d[0] * pow(d[2], -2, R.P) % R.P, d[1] * pow(d[2], -3, R.P) % R.P) == R.add(q, q)
        assert R._jac_add_affine(acc, R.neg(q))[2] == 0


def test_library_table_equals_the_model_and_the_golden_entries():
    from lambda_elliptic_curves_amd import pedersen
    tab = pedersen.table()
    assert tab.shape == (R.N_POINTS, 2, 4) and pedersen.N_POINTS == R.N_POINTS
    assert all(m < R.P for m in R.raw_ints(tab)), "a stored coordinate is not below p"
    assert R.points_from_elems(tab) == R.tables()
    pts = R.points_from_elems(tab)
    for e in golden()["table"]:
        assert pts[e["index"]] == (h(e["x"]), h(e["y"])), (e["table"], e["entry"])
    assert np.array_equal(pedersen.table(), tab)   # generated once, returned again


def test_every_symbol_is_exported():
    from lambda_elliptic_curves_amd import _lib
    import lambda_elliptic_curves_amd as pkg
    L = _lib.lib()
    for sym in SYMBOLS:
        assert sym in _lib.EXPORTS and hasattr(L, sym), sym
        assert getattr(L, sym).argtypes is not None, sym
    assert "pedersen" in pkg.__all__
    for name in ("hash", "hash_device", "commit_leaves", "commit_leaves_device", "table", "add_affine_device"):
        assert callable(getattr(pkg.pedersen, name)), name


def test_argument_codes_need_no_device():
    from lambda_elliptic_curves_amd import _lib
    L = C.CDLL(_lib.LIB_PATH)   # a handle of its own: plain ctypes arguments, no argtypes
    buf = np.zeros(4096, np.uint8)
    assert buf.ctypes.data % 16 == 0
    P, Q, N = C.c_void_p(buf.ctypes.data), C.c_void_p(buf.ctypes.data + 2048), C.c_void_p(None)
    OFF = C.c_void_p(buf.ctypes.data + 8)   # 8-byte aligned only
    i, u32, sz = C.c_int, C.c_uint32, C.c_size_t
    BAD, ALLOC, OK = _lib.ERR_BAD_ARG, _lib.ERR_ALLOC, _lib.OK
    cases = [
        # n = 0: nothing to do, nothing touched (null buffers included)
        ("hash n=0", lambda: L.lw_pedersen_hash(N, N, sz(0), N), OK),
        ("hash_device n=0", lambda: L.lw_pedersen_hash_device(N, N, sz(0), N, N), OK),
        ("add_affine_device n=0", lambda: L.lw_pedersen_add_affine_device(N, N, N, sz(0), N, N), OK),
        # null pointers
        ("hash null x", lambda: L.lw_pedersen_hash(N, P, sz(1), Q), BAD),
        ("hash null y", lambda: L.lw_pedersen_hash(P, N, sz(1), Q), BAD),
        ("hash null out", lambda: L.lw_pedersen_hash(P, P, sz(1), N), BAD),
        ("hash_device null out", lambda: L.lw_pedersen_hash_device(P, P, sz(1), N, N), BAD),
        ("add_affine_device null z", lambda: L.lw_pedersen_add_affine_device(P, N, P, sz(1), Q, N), BAD),
        ("commit null leaves", lambda: L.lw_pedersen_commit_leaves(N, u32(1), u32(2), i(0), P, N), BAD),
        ("commit null root", lambda: L.lw_pedersen_commit_leaves(P, u32(1), u32(2), i(0), N, N), BAD),
        ("commit_device null nodes", lambda: L.lw_pedersen_commit_leaves_device(P, u32(1), u32(2), i(0), N, N, N), BAD),
        ("table null", lambda: L.lw_pedersen_table(N), BAD),
        # misaligned device pointers
        ("hash_device misaligned x", lambda: L.lw_pedersen_hash_device(OFF, P, sz(1), Q, N), BAD),
        ("hash_device misaligned y", lambda: L.lw_pedersen_hash_device(P, OFF, sz(1), Q, N), BAD),
        ("hash_device misaligned out", lambda: L.lw_pedersen_hash_device(P, P, sz(1), OFF, N), BAD),
        ("add_affine_device misaligned q", lambda: L.lw_pedersen_add_affine_device(P, P, OFF, sz(1), Q, N), BAD),
        ("commit_device misaligned leaves", lambda: L.lw_pedersen_commit_leaves_device(OFF, u32(1), u32(2), i(0), Q, N, N), BAD),
        ("commit_device misaligned nodes", lambda: L.lw_pedersen_commit_leaves_device(P, u32(1), u32(2), i(0), OFF, N, N), BAD),
        # a leaf is one element
        ("commit two columns", lambda: L.lw_pedersen_commit_leaves(P, u32(2), u32(2), i(0), Q, N), BAD),
        ("commit no columns", lambda: L.lw_pedersen_commit_leaves(P, u32(0), u32(2), i(0), Q, N), BAD),
        ("commit_device two columns", lambda: L.lw_pedersen_commit_leaves_device(P, u32(2), u32(2), i(0), Q, N, N), BAD),
        # sizes past what can be addressed
        ("commit 2^32 leaves", lambda: L.lw_pedersen_commit_leaves(P, u32(1), u32(32), i(0), Q, N), ALLOC),
        ("commit_device 2^32 leaves", lambda: L.lw_pedersen_commit_leaves_device(P, u32(1), u32(32), i(0), Q, N, N), ALLOC),
        ("hash 2^36 + 1", lambda: L.lw_pedersen_hash(P, P, sz((1 << 36) + 1), Q), ALLOC),
    ]
    got = {name: call() for name, call, _ in cases}
    assert got == {name: code for name, _, code in cases}
    assert not buf.any()


def test_host_forms_fail_loudly_without_a_device():
    import torch
    from lambda_elliptic_curves_amd import errors, pedersen
    one = R.to_elems([1])
    if not torch.cuda.is_available():   # no CPU fallback: with work to do and no device, the host forms raise
        with pytest.raises(errors.HipError):
            pedersen.hash(one, one)
        with pytest.raises(errors.HipError):
            pedersen.commit_leaves(one)
    assert pedersen.hash(np.zeros((0, 4), np.uint64), np.zeros((0, 4), np.uint64)).shape == (0, 4)   # no work: no device needed
    with pytest.raises(errors.InputError):
        pedersen.commit_leaves(np.zeros((3, 4), np.uint64))
    with pytest.raises(errors.HipError):   # two columns: refused before any device work
        pedersen.commit_leaves(np.zeros((2, 4, 4), np.uint64))


def test_host_build_of_the_hash_and_the_group_law_under_sanitizers(tmp_path):
    """pedersen.cuh is host-callable: the table generation runs there in the library, and the hash and the group law
    compile for the host too.  A stand-alone program built with ASan + UBSan hashes the recorded vectors and walks the
    branches of the group law (Z != 1) with the device functions' own source, against the model."""
    src = tmp_path / "t.cpp"
    src.write_text(textwrap.dedent(f"""
        #include <cstdio>
        #include <cstdlib>
        #include <cstring>
        #include <vector>
        struct uint4 {{ unsigned x, y, z, w; }};
        static inline uint4 make_uint4(unsigned a, unsigned b, unsigned c, unsigned d) {{ return uint4{{a, b, c, d}}; }}
        #include "{ROOT}/lambda_elliptic_curves_amd/csrc/pedersen.cuh"
        using namespace lw;
        static SFe parse(const char *hex) {{   // 64 hex digits, a canonical integer -> Montgomery form
            SFe r;
            for (int k = 0; k < 8; k++) {{
                char w[9] = {{0}};
                memcpy(w, hex + 8 * (7 - k), 8);
                r.v[k] = (uint32_t)strtoul(w, nullptr, 16);
            }}
            return fe_to_mont<Stark252>(r);
        }}
        static void show(const SFe &m) {{
            const SFe c = fe_from_mont<Stark252>(m);
            for (int k = 7; k >= 0; k--) printf("%08x", c.v[k]);
        }}
        int main(int argc, char **argv) {{
            std::vector<char> table(PEDERSEN_TABLE_BYTES + 16);
            char *t = table.data() + ((16 - ((size_t)table.data() & 15)) & 15);
            pedersen_fill_table(t);
            int i = 1;
            for (; i + 1 < argc && strcmp(argv[i], "--"); i += 2) {{
                show(pedersen_hash(parse(argv[i]), parse(argv[i + 1]), t));
                printf("\\n");
            }}
            for (i++; i + 4 < argc; i += 5) {{   // px py z qx qy: (p lifted and rescaled by z) + q, p = (0, 0) is infinity
                const SFe px = parse(argv[i]), py = parse(argv[i + 1]), z = parse(argv[i + 2]), z2 = fe_sqr<Stark252>(z);
                const bool inf = px.is_zero() && py.is_zero();
                PedJac acc;
                acc.x = fe_mul<Stark252>(inf ? SFe::one() : px, z2);
                acc.y = fe_mul<Stark252>(inf ? SFe::one() : py, fe_mul<Stark252>(z, z2));
                acc.z = inf ? SFe::zero() : z;
                PedAffine q;
                q.x = parse(argv[i + 3]);
                q.y = parse(argv[i + 4]);
                const PedAffine r = ped_to_affine(ped_add_affine(acc, q));
                show(r.x);
                printf(" ");
                show(r.y);
                printf("\\n");
            }}
            return 0;
        }}
    """))
    exe = tmp_path / "t"
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", str(exe), str(src)])
    hx = lambda v: "%064x" % v
    hashes = [(h(c["x"]), h(c["y"])) for c in golden()["hash"]] + [((1 << 248) - 1, 1 << 251), (1 << 244, 0)]
    t = R.tables()
    a, b = t[7], t[1234]
    rows = [(p, z, q) for z in (1, 2, R.P - 1, 0x1234567)
            for p, q in ((a, b), (a, a), (a, R.neg(a)), (None, b), (R.P0, t[0]))]
    args = [hx(v) for pair in hashes for v in pair] + ["--"]
    for p, z, q in rows:
        args += [hx(v) for v in ((p or (0, 0)) + (z,) + q)]
    out = subprocess.run([str(exe)] + args, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = out.stdout.split("\n")[:-1]
    assert len(lines) == len(hashes) + len(rows)
    assert [int(ln, 16) for ln in lines[:len(hashes)]] == [R.hash(x, y) for x, y in hashes]
    for ln, (p, z, q) in zip(lines[len(hashes):], rows):
        got = tuple(int(w, 16) for w in ln.split())
        assert got == (R.add(p, q) or (0, 0)), (p, z, q)
