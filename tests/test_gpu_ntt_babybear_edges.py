"""GPU parity for the BabyBear NTT (csrc/ntt_bb.hip) where seeded random residues do not reach: operands at the edges of
the value range, the coset tables above 2^13, every compiled tile shape in every form, a cold and a warm twiddle cache.
Bytes are compared, in all three layouts (u32 R = 2^32, u64 R = 2^64, quartic-extension values), through
lw_hip_ntt_device / lw_hip_ntt_lde_device; the output buffer is poisoned before each run.

Inputs are stored words as the memory holds them (any word below p is a legal element in every layout): every word
p - 1; a single p - 1 at index n/3 among zeros; 0 and p - 1 alternating; one seeded random vector.  A butterfly sum that
lands exactly on p or on 0, which random data meets with probability 2^-31 per addition, is the rule with these.  The
four components of an extension vector carry the four kinds, rotated per case, so that a component mix-up cannot hide.

Sizes: tests/ntt_bb_cases.py — tests/test_ntt_bb_shapes_cpu.py shows without a device that they reach every
instantiation of bb_pass_kernel<LAST, IN64, OUT64, RX, VX> a buffer of 2^20 words can reach (L = 12 is the largest size
with run-time tile shapes only; the first compiled middle pass is L = 20, for the extension L = 17; a single pass with a
compiled shape exists only as a low-degree extension with blow-up 32 and more, the extension: 8).  A compiled middle
pass of 8 stages needs 2^23 words and is left to test_max_size_2_24_roundtrip_u32.  From 2^18 words on only `all-p-1`
and `random` (the extension: two of the four rotations) run in every form.

Forms: forward, inverse, both on a coset, the low-degree extension on a coset; all but the last into a second buffer
and in place.  Coset offsets: 7, and p - 1, whose powers alternate 1 and p - 1.

Two references: the CPU oracle for every case, and closed forms in plain integers that do not go through the oracle's C
code (the transform is linear over the stored words with canonical twiddles, whatever the Montgomery radix):
  an impulse v at index j, forward on the coset h:            out[k] = v (h w^k)^j
  an impulse v at evaluation index k0, inverse on the coset h: out[j] = v n^-1 h^-j w^(-j k0)
  a constant c, forward:                                       out[0] = n c, zero elsewhere
with j, k0 in {n/3, n - 1}: n - 1 reaches the last entry of both levels of the coset tables, and the inverse impulse pins
every entry of the inverse tables (N^-1 folded into the upper level) one by one."""
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import bigint_def as D
from oracle import oracle as O
from tests import ntt_bb_cases as cases
from tests import util

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

P = D.P_BABYBEAR
LGV = {"babybear_u32": 0, "babybear_u64": 0, "babybear_ext4": 2}
KINDS = ("all-p-1", "one-p-1", "alternating", "random")
OFFSETS = {"7": 7, "p-1": P - 1}
PLAIN_FORMS = [("forward", None), ("inverse", None), ("coset-forward", "7"), ("coset-forward", "p-1"), ("coset-inverse", "7"),
               ("coset-inverse", "p-1")]
POISON = {np.dtype(np.uint32): 0xA5A5A5A5 - (1 << 32), np.dtype(np.uint64): -0x0123456789abcdef}   # as signed words; neither is below p
_CACHE_UP_TO = 16   # in log2 words: these also serve the batched cases; larger results are used once and not kept
_inputs, _expecteds = {}, {}


def _dtype(name):
    return np.dtype(np.uint32 if name == "babybear_u32" else np.uint64)


def _words(kind, n, dtype, seed):
    """n stored words of one kind"""
    if kind == "random":
        return np.random.default_rng(seed).integers(0, P, size=n, dtype=dtype)
    a = np.zeros(n, dtype)
    a[{"all-p-1": slice(None), "one-p-1": slice(n // 3, n // 3 + 1), "alternating": slice(1, None, 2)}[kind]] = P - 1
    return a


def _kinds(name, log_n):
    """the kinds that run at a size: names for the base field, rotations of the four names over the components for the extension"""
    reduced = log_n + LGV[name] >= cases.REDUCED_FROM_LOG_WORDS
    if name == "babybear_ext4":
        return (0, 2) if reduced else (0, 1, 2, 3)
    return ("all-p-1", "random") if reduced else KINDS


def _input(name, kind, log_n):
    key = (name, kind, log_n)
    if key not in _inputs:
        n = 1 << log_n
        if name == "babybear_ext4":
            a = np.stack([_words(KINDS[(kind + k) % 4], n, _dtype(name), 8100 + 4 * log_n + k) for k in range(4)], axis=1)
        else:
            a = _words(kind, n, _dtype(name), 8000 + log_n)
        a.setflags(write=False)
        if log_n + LGV[name] > _CACHE_UP_TO:
            return a
        _inputs[key] = a
    return _inputs[key]


def _offset(name, off):
    return None if off is None else util.offset_elem(name, OFFSETS[off])


def _expected(name, kind, log_n, skip, form, off):
    key = (name, kind, log_n, skip, form, off)
    if key in _expecteds:
        return _expecteds[key]
    oid = util.field_pairs()[name][1]
    a = _input(name, kind, log_n - skip)
    if form in ("inverse", "coset-inverse"):
        exp = O.interpolate_fft(oid, a, _offset(name, off))
    else:   # zero padded to the domain, whatever the polynomial's degree: the device transforms all n words
        exp = O.evaluate_fft(oid, a, 1 << skip, a.shape[0], _offset(name, off))
    exp = exp.reshape((1 << log_n,) + a.shape[1:])
    if log_n + LGV[name] <= _CACHE_UP_TO:
        exp.setflags(write=False)
        _expecteds[key] = exp
    return exp


def _run(name, form, log_n, skip, a, off, batch=1, in_place=False):
    """`a`: batch blocks of input, densely packed.  Returns the batch outputs, densely packed, and the input buffer afterwards."""
    import torch
    from lambda_elliptic_curves_amd import fft
    fld = util.field_pairs()[name][0]
    sdt = np.int32 if a.dtype == np.uint32 else np.int64
    t_in = torch.from_numpy(np.array(a).view(sdt)).cuda()   # a copy: the shared inputs are read-only
    if in_place:
        t_out = t_in
    else:
        t_out = torch.full((batch << (log_n + LGV[name]),), POISON[a.dtype], dtype=t_in.dtype, device="cuda")
    if skip:
        fft.lde_device(fld, t_in, log_n - skip, t_out, log_n, batch=batch, offset=_offset(name, off))
    else:
        fft.ntt_device(fld, t_in, t_out, log_n, inverse=form in ("inverse", "coset-inverse"), batch=batch, batch_stride=1 << log_n,
                       offset=_offset(name, off))
    torch.cuda.synchronize()
    back = lambda t: t.cpu().numpy().view(a.dtype).reshape((-1,) + a.shape[1:])
    return back(t_out), back(t_in)


def _assert_same(got, exp, what):
    got, exp = np.asarray(got), np.asarray(exp)
    assert got.dtype == exp.dtype and got.size == exp.size, what
    if got.tobytes() != exp.tobytes():
        bad = np.flatnonzero(got.reshape(-1) != exp.reshape(-1))
        i = int(bad[0])
        raise AssertionError(f"{what}: {bad.size} of {got.size} words differ, first at word {i}: got {int(got.reshape(-1)[i])}, "
                             f"expected {int(exp.reshape(-1)[i])}")


def _plain_cases():
    out = []
    for name in LGV:
        for log_n, _ in cases.sizes(LGV[name], False):
            out += [pytest.param(name, log_n, form, off, id=f"{name}-{log_n}-{form}" + (f"-{off}" if off else "")) for form, off in PLAIN_FORMS]
    return out


def _lde_cases():
    return [pytest.param(name, log_n, skip, off, id=f"{name}-{log_n}-skip{skip}-{off}")
            for name in LGV for log_n, skip in cases.sizes(LGV[name], True) for off in OFFSETS]


@pytest.mark.parametrize("name,log_n,form,off", _plain_cases())
def test_matches_oracle(name, log_n, form, off):
    for kind in _kinds(name, log_n):
        a = _input(name, kind, log_n)
        exp = _expected(name, kind, log_n, 0, form, off)
        got, after = _run(name, form, log_n, 0, a, off)
        _assert_same(got, exp, (kind, "distinct"))
        _assert_same(after, a, (kind, "the input of a run into a second buffer"))
        got, _ = _run(name, form, log_n, 0, a, off, in_place=True)
        _assert_same(got, exp, (kind, "in place"))


@pytest.mark.parametrize("name,log_n,skip,off", _lde_cases())
def test_low_degree_extension_matches_oracle(name, log_n, skip, off):
    for kind in _kinds(name, log_n):
        a = _input(name, kind, log_n - skip)
        got, after = _run(name, "lde", log_n, skip, a, off)
        _assert_same(got, _expected(name, kind, log_n, skip, "lde", off), kind)
        _assert_same(after, a, (kind, "input"))


@pytest.mark.parametrize("first", (0, 1))
@pytest.mark.parametrize("name", list(LGV))
def test_low_degree_extension_batch_of_three_at_a_compiled_first_pass(name, first):
    """three blocks of different kinds in one launch (the extension: three rotations); the first pass is an RX = 8 (the
    extension: RX = 6) kernel whose blockIdx.y picks the block"""
    log_n, skip = (13, 2) if name == "babybear_ext4" else (16, 1)
    assert (LGV[name], log_n, skip) in cases.SIZES
    all_kinds = (0, 1, 2, 3) if name == "babybear_ext4" else KINDS
    kinds = [all_kinds[(first + b) % 4] for b in range(3)]
    a = np.concatenate([_input(name, k, log_n - skip) for k in kinds])
    got, after = _run(name, "lde", log_n, skip, a, "7", batch=3)
    _assert_same(after, a, "input")
    for b, k in enumerate(kinds):
        _assert_same(got[b << log_n:(b + 1) << log_n], _expected(name, k, log_n, skip, "lde", "7"), (b, k))


# ---------------------------------------------------------------- closed forms
_pows = {}


def _powers(base, n):
    """base^0 .. base^(n-1) mod p, one product at a time in Python integers"""
    key = (base, n)
    if key not in _pows:
        out, x = [0] * n, 1
        for i in range(n):
            out[i] = x
            x = x * base % P
        _pows[key] = np.array(out, np.uint64)
        _pows[key].setflags(write=False)
    return _pows[key]


def _mulmod(a, b):
    """(a * b) mod p on uint64 arrays of residues: the products stay below 2^62"""
    return (np.asarray(a, np.uint64) * np.asarray(b, np.uint64)) % np.uint64(P)


def _impulse_forward(n, w, h, j, v):
    k = np.arange(n, dtype=np.uint64)
    return _mulmod(v * pow(h, j, P) % P, _powers(w, n)[(np.uint64(j) * k) % np.uint64(n)])


def _impulse_inverse(n, w, h, k0, v):
    j = np.arange(n, dtype=np.uint64)
    w_inv_jk0 = _powers(w, n)[(np.uint64(n) - (j * np.uint64(k0)) % np.uint64(n)) % np.uint64(n)]
    return _mulmod(_mulmod(v * pow(n, -1, P) % P, _powers(pow(h, -1, P), n)), w_inv_jk0)


IMPULSES = lambda n: ((n // 3, P - 1), (n - 1, P - 1), (n // 3, 1), (n - 1, 123456789))


@pytest.mark.parametrize("off", [None, "7", "p-1"])
@pytest.mark.parametrize("name,log_n", [(name, log_n) for name in LGV for log_n in ((13, 16) if LGV[name] else (13, 16, 18))])
def test_closed_forms(name, log_n, off):
    n, dt = 1 << log_n, _dtype(name)
    w = D.primitive_root_of_unity(P, log_n)
    h = OFFSETS[off] if off else 1
    assert pow(w, n, P) == 1 and pow(w, n // 2, P) == P - 1
    imp = IMPULSES(n)
    # the columns of a run: the base field runs one impulse at a time, the extension all four at once, one per component, in two rotations
    runs = [[imp[(r + k) % 4] for k in range(4)] for r in (0, 1)] if name == "babybear_ext4" else [[iv] for iv in imp]
    for run in runs:
        a = np.zeros((n, len(run)), dt)
        for k, (pos, v) in enumerate(run):
            a[pos, k] = v
        a = a if name == "babybear_ext4" else a.reshape(n)
        for inverse, closed in ((False, _impulse_forward), (True, _impulse_inverse)):
            exp = np.stack([closed(n, w, h, pos, v) for pos, v in run], axis=1).astype(dt).reshape(a.shape)
            form = ("coset-" if off else "") + ("inverse" if inverse else "forward")
            got, _ = _run(name, form, log_n, 0, a, off)
            _assert_same(got, exp, (form, run))
    if off is None:
        consts = (P - 1, 1, 12345, P - 2) if name == "babybear_ext4" else (P - 1,)
        a = np.tile(np.array(consts, dt), (n, 1))
        exp = np.zeros_like(a)
        exp[0] = [n * c % P for c in consts]
        a, exp = (a, exp) if name == "babybear_ext4" else (a.reshape(n), exp.reshape(n))
        got, _ = _run(name, "forward", log_n, 0, a, None)
        _assert_same(got, exp, "constant")


# ---------------------------------------------------------------- twiddle cache
WARM_SIZES = (16, 5, 13, 18, 13, 20, 5)
WARM_CHILD = r"""
import sys
import numpy as np
import torch
from lambda_elliptic_curves_amd import fft
from oracle import oracle as O
from tests import util
sizes = [int(v) for v in sys.argv[1].split(",")]
bad = 0
for step, log_n in enumerate(sizes):
    for name in ("babybear_u32", "babybear_u64"):
        fld, oid = util.field_pairs()[name]
        off = util.offset_elem(name, 7)
        a = util.rand_elems(name, 1 << log_n, 8800 + log_n)
        a[-1] |= 1
        for form, inverse, offset in (("forward", False, None), ("inverse", True, None), ("coset-inverse", True, off)):
            exp = O.interpolate_fft(oid, a, offset) if inverse else O.evaluate_fft(oid, a, 1, a.shape[0], offset)
            t_in = torch.from_numpy(a.view(np.int32 if a.dtype == np.uint32 else np.int64).copy()).cuda()
            t_out = torch.full_like(t_in, -0x5a5a5a5b)
            fft.ntt_device(fld, t_in, t_out, log_n, inverse=inverse, offset=offset)
            torch.cuda.synchronize()
            ok = t_out.cpu().numpy().view(a.dtype).tobytes() == np.ascontiguousarray(exp).tobytes()
            bad += not ok
            print("step", step, log_n, name, form, "ok" if ok else "DIFFERS", flush=True)
sys.exit(1 if bad else 0)
"""


def test_warm_cache_grows_and_shrinks():
    """The twiddle table (T | dd, dd located from the CACHED table's size) is kept between calls and grows by reallocation.
    A fresh process makes the sequence independent of what ran before: 2^16 cold, 2^5 and 2^13 against a larger cached
    table, the growth steps 16 -> 18 and 18 -> 20, and smaller transforms after each.  Forward and inverse tables are
    separate; u32 and u64 share them.  One child, started once."""
    out = subprocess.run([sys.executable] + (["-s"] if sys.flags.no_user_site else []) + ["-c", WARM_CHILD, ",".join(str(s) for s in WARM_SIZES)],
                         cwd=ROOT, capture_output=True, text=True, timeout=240)
    lines = [line for line in out.stdout.splitlines() if line.startswith("step ")]
    want = [f"step {i} {log_n} {name} {form} ok" for i, log_n in enumerate(WARM_SIZES) for name in ("babybear_u32", "babybear_u64")
            for form in ("forward", "inverse", "coset-inverse")]
    assert lines == want, (out.stdout[-2000:], out.stderr[-2000:])
    assert out.returncode == 0, out.stderr[-2000:]
