"""The host tables of csrc/ext_steps.cuh without a device: the power tables of a point, the regrouping of the DEEP weights
into groups of four points and the constants c_j, under both policies (Fp2 over Goldilocks, Fp4 over BabyBear), compiled
for the host with the address and undefined-behaviour sanitizers (tests/ext_steps_host_main.cpp), run as a child process
and compared word for word with the Python models."""
import os
import subprocess

import numpy as np
import pytest

from tests import babybear_ext_ref as B
from tests import goldilocks_ext_ref as X

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_COEFFS, STEPS, TILE, PTS, N_COLS = 8, 8, 2048, 4, 3
GROUPS, MS = (1, 2, 257), (1, 4, 5)


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    hipcc = "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        hipcc = "hipcc"
    out = tmp_path_factory.mktemp("ext_steps") / "ext_steps_host"
    subprocess.check_call([hipcc, "-x", "hip", "--cuda-host-only", "-O2", "-std=c++17", "-Xarch_host", "-fsanitize=address,undefined",
                           "-Xarch_host", "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "lambda_elliptic_curves_amd", "csrc"),
                           os.path.join(ROOT, "tests", "ext_steps_host_main.cpp"), "-o", str(out)], timeout=600)
    return str(out)


def expected(F, points, tables):
    """the lines of the program, elements of the model F in: F.power, F.mul, F.add"""
    want = []
    for x in points:
        for group in GROUPS:
            want += [F.power(x, e) for e in range(E_COEFFS)]
            want += [F.power(x, E_COEFFS << s) for s in range(STEPS)]
            want.append(F.power(x, TILE))
            want += [F.power(x, (TILE * group) << s) for s in range(STEPS)]
    zero = F.sub(points[0], points[0])
    for m, (weights, evals) in zip(MS, tables):
        for g in range((m + PTS - 1) // PTS):
            for k in range(N_COLS):
                want += [weights[k * m + PTS * g + j] if PTS * g + j < m else zero for j in range(PTS)]
        for j in range(m):
            c = zero
            for k in range(N_COLS):
                c = F.add(c, F.mul(weights[k * m + j], evals[k * m + j]))
            want.append(c)
    return want


def run(exe, name, points, tables):
    """points and tables as the words handed to the calls -> the printed lines as tuples of words"""
    words = [w for p in points for w in p]
    for weights, evals in tables:
        words += [w for s in weights + evals for w in s]
    out = subprocess.run([exe, name, str(len(points))] + [str(w) for w in words], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    return [tuple(int(w) for w in line.split()) for line in out.stdout.splitlines()]


def test_goldilocks_fp2_tables(exe):
    P = X.P
    rng = np.random.default_rng(101)
    rand = lambda n: [tuple(int(v) for v in row) for row in rng.integers(0, 1 << 64, (n, 2), dtype=np.uint64)]   # any u64
    points = [(P - 1, P - 1), (0, 1), (3, 5), (P, (1 << 64) - 1)] + rand(2)
    tables = [(rand(N_COLS * m), rand(N_COLS * m)) for m in MS]
    tables[1][0][5], tables[2][1][0] = (P, P + 1), ((1 << 64) - 1, 0)   # words that are not canonical
    got = run(exe, "gl2", points, tables)
    want = expected(X, [X.elem(p) for p in points], [([X.elem(s) for s in w], [X.elem(s) for s in e]) for w, e in tables])
    assert len(want) == len(points) * len(GROUPS) * 25 + sum(((m + 3) // 4) * 12 + m for m in MS)
    assert got == want


def test_babybear_fp4_tables(exe):
    P = B.P
    rng = np.random.default_rng(102)
    rand = lambda n: [tuple(int(v) for v in row) for row in rng.integers(0, P, (n, 4))]   # stored words, below p
    points = [(P - 1,) * 4, (0, B.store(1), 0, 0), B.store_elem((3, 5, 7, 9)), tuple(B.EDGE[4:])] + rand(2)
    tables = [(rand(N_COLS * m), rand(N_COLS * m)) for m in MS]
    tables[1][0][5], tables[2][1][0] = (P - 1,) * 4, (0,) * 4
    got = run(exe, "bb4", points, tables)
    un = lambda scalars: [B.unstore_elem(s) for s in scalars]
    want = expected(B, un(points), [(un(w), un(e)) for w, e in tables])
    assert got == [B.store_elem(v) for v in want]
