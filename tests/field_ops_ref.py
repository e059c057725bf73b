"""Plain-integer reference of the primitives of csrc/field.cuh, one function per op of lw_hip_field_pointwise_device, and
the operand sets of tests/test_field_pointwise_cpu.py and tests/test_gpu_field_pointwise.py.

Everything is on stored integers (for the Montgomery fields: the residue times R, as it sits in memory).  The raw lazy
product is the exact integer the FIPS columns form, t = (a*b + ((-a*b*p^-1) mod R) * p) / R; everything canonical is the
obvious % p.  Every operand set stays inside the domain csrc/field_pointwise_ops.cuh documents for its op."""
import functools
import itertools
import random

import numpy as np

from tests import ec_formulas_ref as E

(OP_ADD, OP_SUB, OP_NEG, OP_DBL, OP_MUL, OP_SQR, OP_MUL_LAZY, OP_MUL_LAZY_UNIFORM, OP_REDUCE_FULL, OP_COND_SUB_P, OP_ADD_RAW,
 OP_ADD2P_SUB_RAW, OP_NEG_RAW, OP_NEG_RAW_2P, OP_TO_MONT, OP_FROM_MONT, OP_DOT2, OP_DOT4, OP_INV, OP_REDUCE64, OP_FROM_R64,
 OP_TO_R64) = range(22)   # lw_field_op_t
OP_NAMES = ["add", "sub", "neg", "dbl", "mul", "sqr", "mul_lazy", "mul_lazy_uniform", "reduce_full", "cond_sub_p", "add_raw",
            "add2p_sub_raw", "neg_raw", "neg_raw_2p", "to_mont", "from_mont", "dot2", "dot4", "inv", "reduce64", "from_r64", "to_r64"]
TWO_OPERANDS = {OP_ADD, OP_SUB, OP_MUL, OP_MUL_LAZY, OP_MUL_LAZY_UNIFORM, OP_ADD_RAW, OP_ADD2P_SUB_RAW, OP_DOT2, OP_DOT4}
CANONICAL = {OP_ADD, OP_SUB, OP_NEG, OP_DBL, OP_MUL, OP_SQR, OP_REDUCE_FULL, OP_TO_MONT, OP_FROM_MONT, OP_DOT2, OP_DOT4, OP_INV}
ROW_ELEMS = {OP_DOT2: 2, OP_DOT4: 4}
N_RANDOM = 4096
N_EACH_SIDE = 16          # rows on either side of the final subtraction that the product ops must have


class Field:
    """pw: lw_pw_field_t; words: u64 limbs of a stored element; oracle: the oracle's field id"""

    def __init__(self, name, pw, p, words, oracle):
        self.name, self.pw, self.p, self.words, self.oracle = name, pw, p, words, oracle
        self.R = 1 << (64 * words)
        self.Rinv = pow(self.R, -1, p)
        self.pinv = pow(p, -1, self.R)
        self.top = p >> (64 * words - 32)          # p's top 32-bit limb

    def __repr__(self):
        return self.name

    def has(self, op):
        if op > OP_INV:
            return False
        return ROW_ELEMS.get(op, 1) * (self.top + 1) <= 1 << 32     # the static_assert of fe_dot (KSUM = P)


STARK252 = Field("stark252", 0, (1 << 251) + 17 * (1 << 192) + 1, 4, 0)
FR381 = Field("fr381", 1, 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001, 4, 1)
FR254 = Field("fr254", 2, 21888242871839275222246405745257275088548364400416034343698204186575808495617, 4, 7)
FP381 = Field("fp381", 3, 0x1a0111ea397fe69a4b1ba7b6434bacd764774b84f38512bf6730d2a0f6b0f6241eabfffeb153ffffb9feffffffffaaab, 6, 5)
FP254 = Field("fp254", 4, 21888242871839275222246405745257275088696311157297823662689037894645226208583, 4, 6)
FIELDS = [STARK252, FR381, FR254, FP381, FP254]
BY_NAME = {f.name: f for f in FIELDS}
FIELD_OPS = [op for op in range(OP_INV + 1)]
PW_FIELD_BABYBEAR = 5

A_TOP = (1 << 251) + 16 * (1 << 192) + ((1 << 192) - 1)     # Stark252: a[7] = 2^27 at its bound, a[6] = 16, lower limbs all ones


# ---------------------------------------------------------------- the ops
def lazy(f, s):
    """the unreduced Montgomery quotient of the integer s (a product or a sum of products)"""
    q, rem = divmod(s + ((-s * f.pinv) % f.R) * f.p, f.R)
    assert rem == 0
    return q


def op_add(f, a, b): return (a + b) % f.p
def op_sub(f, a, b): return (a - b) % f.p
def op_neg(f, a): return (-a) % f.p
def op_dbl(f, a): return 2 * a % f.p
def op_mul(f, a, b): return a * b * f.Rinv % f.p
def op_sqr(f, a): return a * a * f.Rinv % f.p
def op_mul_lazy(f, a, b): return lazy(f, a * b)
def op_reduce_full(f, a): return a % f.p
def op_cond_sub_p(f, a): return a - f.p if a >= f.p else a
def op_add_raw(f, a, b): return a + b
def op_add2p_sub_raw(f, a, b): return a + 2 * f.p - b
def op_neg_raw(f, a): return f.p - a
def op_neg_raw_2p(f, a): return 2 * f.p - a
def op_to_mont(f, a): return a * f.R % f.p
def op_from_mont(f, a): return a * f.Rinv % f.p
def op_dot(f, a, b): return sum(x * y for x, y in zip(a, b)) * f.Rinv % f.p
def op_inv(f, a): return pow(a, f.p - 2, f.p) * f.R * f.R % f.p      # (a / R)^-1 * R


OPS = {OP_ADD: op_add, OP_SUB: op_sub, OP_NEG: op_neg, OP_DBL: op_dbl, OP_MUL: op_mul, OP_SQR: op_sqr, OP_MUL_LAZY: op_mul_lazy,
       OP_MUL_LAZY_UNIFORM: op_mul_lazy, OP_REDUCE_FULL: op_reduce_full, OP_COND_SUB_P: op_cond_sub_p, OP_ADD_RAW: op_add_raw,
       OP_ADD2P_SUB_RAW: op_add2p_sub_raw, OP_NEG_RAW: op_neg_raw, OP_NEG_RAW_2P: op_neg_raw_2p, OP_TO_MONT: op_to_mont,
       OP_FROM_MONT: op_from_mont, OP_DOT2: op_dot, OP_DOT4: op_dot, OP_INV: op_inv}


def in_domain(f, op, a, b=None):
    """the operand domain of csrc/field_pointwise_ops.cuh"""
    p, R = f.p, f.R
    if op in (OP_DOT2, OP_DOT4):
        return len(a) == len(b) == ROW_ELEMS[op] and all(0 <= v <= p for v in a + b)
    if not 0 <= a < R or (b is not None and not 0 <= b < R) or (b is None) == (op in TWO_OPERANDS):
        return False
    if op in (OP_ADD, OP_SUB):
        return a < p and b < p
    if op == OP_MUL:
        return a < p or b < p
    if op in (OP_MUL_LAZY, OP_MUL_LAZY_UNIFORM, OP_NEG, OP_DBL, OP_SQR, OP_TO_MONT, OP_FROM_MONT, OP_INV):
        return a < p
    if op == OP_REDUCE_FULL:
        return f is STARK252 or a < 2 * p
    if op == OP_ADD_RAW:
        return a + b < R
    if op == OP_ADD2P_SUB_RAW:
        return b <= a + 2 * p and a + 2 * p - b < R
    if op == OP_NEG_RAW:
        return a <= p
    if op == OP_NEG_RAW_2P:
        return a <= 2 * p
    return op == OP_COND_SUB_P


# ---------------------------------------------------------------- operand sets
@functools.lru_cache(maxsize=None)
def edge_set(name):
    """E: the edge values of ec_formulas_ref (31 for a 4-word field), the dense-ones value below p's top bit (Stark252:
    2^251 - 1) and, for Stark252, A_TOP: the operands of tests/test_gpu_stark252_lazy_mul_bounds.py.  All < p."""
    f = BY_NAME[name]
    e = E.edge_values(f.p, f.words, 11) + [(1 << (f.p.bit_length() - 1)) - 1]
    if f is STARK252:
        e.append(A_TOP)
    e = list(dict.fromkeys(e))                    # in order, without the few values that coincide (2 = 2^1 ...)
    assert all(v < f.p for v in e)
    return e


@functools.lru_cache(maxsize=None)
def wide_set(name):
    """E': E and the values at and above p, for the operands that may be any N-limb value"""
    f = BY_NAME[name]
    p = f.p
    out = [v for v in (p, p + 1, 2 * p - 1, 2 * p, 11 * p - 1, 17 * p - 1, 24 * p - 1, f.R - 1) if v < f.R]   # R - 1: every limb 0xffffffff
    return edge_set(name) + out


def stark_reduction_inputs():
    """-> (borrow, others): the 93 inputs q*p - 1, q*2^251, q*2^251 + 1 (q = 1..31) at which x >> 251 is one more than
    floor(x / p) and the conditional + p fires; q*2^251 - 1 for q = 1..32 (the largest value of every quotient estimate, 2^256 - 1
    the last), and q*p, q*p + 1"""
    p = STARK252.p
    borrow = [v for q in range(1, 32) for v in (q * p - 1, q << 251, (q << 251) + 1)]
    others = [(q << 251) - 1 for q in range(1, 33)] + [v for q in range(1, 32) for v in (q * p, q * p + 1)]
    return borrow, others


def _searched_products(f, op, rng):
    """N_EACH_SIDE rows with the unreduced product at or above p and as many below it (uniform operands, fixed seed): the
    final subtraction is taken by under 1 % of Stark252's pairs"""
    hi, lo = [], []
    while len(hi) < N_EACH_SIDE or len(lo) < N_EACH_SIDE:
        a = rng.randrange(f.p)
        b = a if op == OP_SQR else rng.randrange(f.p)
        side = hi if lazy(f, a * b) >= f.p else lo
        if len(side) < N_EACH_SIDE:
            side.append((a, b))
    return hi + lo


@functools.lru_cache(maxsize=None)
def operands(name, op):
    """-> (a_rows, b_rows or None): the targeted rows first, then N_RANDOM rows drawn half from the sets and half
    uniformly: of a row's two operands one is a member of the set and the other uniform, in turns (for an op with one
    operand: every other row), so that no random row repeats a targeted pair and the two kinds can be told apart
    (test_targeted_rows_reach_further_...).  A DOT row is a tuple of 2 / 4 integers."""
    f = BY_NAME[name]
    assert f.has(op) and op != OP_MUL_LAZY_UNIFORM
    p, R = f.p, f.R
    ed, wd = edge_set(name), wide_set(name)
    rng = random.Random(7000 + 100 * f.pw + op)
    below_p = lambda member: rng.choice(ed) if member else rng.randrange(p)
    any_limbs = lambda member: rng.choice(wd) if member else rng.randrange(R)
    turns = [i % 2 == 0 for i in range(N_RANDOM)]
    if op in (OP_ADD, OP_SUB):
        rows = list(itertools.product(ed, ed)) + [(below_p(s), below_p(not s)) for s in turns]
    elif op == OP_MUL:          # the canonical operand first, then second
        rows = list(itertools.product(ed, wd)) + [(b, a) for a, b in itertools.product(ed, wd)] + _searched_products(f, op, rng)
        rows += [(below_p(s), any_limbs(not s))[::1 if i % 4 < 2 else -1] for i, s in enumerate(turns)]
    elif op == OP_MUL_LAZY:
        rows = list(itertools.product(ed, wd)) + _searched_products(f, op, rng) + [(below_p(s), any_limbs(not s)) for s in turns]
    elif op == OP_SQR:
        rows = [(a, None) for a in ed] + [(a, None) for a, _ in _searched_products(f, op, rng)] + [(below_p(s), None) for s in turns]
    elif op in (OP_NEG, OP_DBL, OP_TO_MONT, OP_FROM_MONT, OP_INV):
        rows = [(a, None) for a in ed] + [(below_p(s), None) for s in turns]
    elif op == OP_NEG_RAW:
        rows = [(a, None) for a in ed + [p]] + [(below_p(s), None) for s in turns]
    elif op == OP_NEG_RAW_2P or (op == OP_REDUCE_FULL and f is not STARK252):
        top = [p, p + 1, 2 * p - 1] + ([2 * p] if op == OP_NEG_RAW_2P else [])
        rows = [(a, None) for a in ed + top] + [(rng.choice(ed + top) if s else rng.randrange(2 * p), None) for s in turns]
    elif op == OP_REDUCE_FULL:
        borrow, others = stark_reduction_inputs()
        rows = [(a, None) for a in wd + borrow + others] + [(any_limbs(s), None) for s in turns]
    elif op == OP_COND_SUB_P:
        rows = [(a, None) for a in wd] + [(any_limbs(s), None) for s in turns]
    elif op == OP_ADD_RAW:
        rows = [(a, b) for a, b in itertools.product(wd, wd) if a + b < R]
        for s in turns:
            a = any_limbs(s)
            rows.append((a, rng.randrange(R - a)))
    elif op == OP_ADD2P_SUB_RAW:
        rows = [(a, b) for a, b in itertools.product(wd, wd) if in_domain(f, op, a, b)]
        rows += [(a, a + 2 * p) for a in wd if a + 2 * p < R]                  # b == a + 2p: the result is 0
        for s in turns:
            a = any_limbs(s)
            rows.append((a, rng.randrange(max(0, a + 2 * p - R + 1), min(R - 1, a + 2 * p) + 1)))
    else:                       # DOT2, DOT4: operands <= p
        k = ROW_ELEMS[op]
        ep = ed + [p]
        pairs = list(itertools.product(ep, ep))
        # every pair of E u {p} as the first product; the other products walk the same list with strides coprime to its length
        rows = [tuple(zip(*(pairs[(i + q * (7 * q + 4)) % len(pairs)] for q in range(k)))) for i in range(len(pairs))]
        z = (0,) * (k - 1)
        rows += [((a,) + z, (p,) + z) for a in ed if a] + [((p,) + z, (a,) + z) for a in ed if a]    # the unreduced sum is exactly p
        rows += [((p,) * k, (p,) * k), ((p - 1,) * k, (p - 1,) * k), ((p,) * k, (p - 1,) * k)]
        draw = lambda member: rng.choice(ep) if member else rng.randrange(p)
        rows += [(tuple(draw((q % 2 == 0) == s) for q in range(k)), tuple(draw((q % 2 == 0) != s) for q in range(k))) for s in turns]
    a_rows = [r[0] for r in rows]
    b_rows = [r[1] for r in rows] if op in TWO_OPERANDS else None
    assert all(in_domain(f, op, a, b_rows[i] if b_rows else None) for i, a in enumerate(a_rows)), (name, op)
    return a_rows, b_rows


@functools.lru_cache(maxsize=None)
def expected(name, op):
    f = BY_NAME[name]
    a_rows, b_rows = operands(name, op)
    fn = OPS[op]
    return [fn(f, a, b_rows[i]) if b_rows else fn(f, a) for i, a in enumerate(a_rows)]


def n_targeted(name, op):
    return len(operands(name, op)[0]) - N_RANDOM


# ---------------------------------------------------------------- packing: u64 limbs, most significant first
def pack(f, vals):
    """integers -> (len, words) uint64"""
    nb = 8 * f.words
    return np.frombuffer(b"".join(v.to_bytes(nb, "big") for v in vals), dtype=">u8").astype(np.uint64).reshape(-1, f.words)


def pack_rows(f, rows):
    """rows of integers, or of tuples of integers (DOT) -> (len, words per row) uint64"""
    if rows and isinstance(rows[0], tuple):
        return pack(f, [v for r in rows for v in r]).reshape(len(rows), -1)
    return pack(f, rows)


def unpack(f, arr):
    nb = 8 * f.words
    raw = np.ascontiguousarray(arr, dtype=np.uint64).astype(">u8").tobytes()
    return [int.from_bytes(raw[i:i + nb], "big") for i in range(0, len(raw), nb)]


# ---------------------------------------------------------------- BabyBear
BB_P = 2013265921
BB_R = 1 << 32
BB_OPS = [OP_MUL, OP_ADD, OP_SUB, OP_REDUCE64, OP_FROM_R64, OP_TO_R64]
BB_IN_DTYPE = {OP_MUL: np.uint32, OP_ADD: np.uint32, OP_SUB: np.uint32, OP_TO_R64: np.uint32, OP_REDUCE64: np.uint64, OP_FROM_R64: np.uint64}
BB_OUT_DTYPE = {op: (np.uint64 if op == OP_TO_R64 else np.uint32) for op in BB_OPS}


def bb_reduce_raw(x):
    """(x + m*p) / 2^32 before the final min, as bb_reduce forms it"""
    m = (-x * pow(BB_P, -1, BB_R)) % BB_R
    q, rem = divmod(x + m * BB_P, BB_R)
    assert rem == 0
    return q


def bb_op(op, a, b=None):
    rinv = pow(BB_R, -1, BB_P)
    if op == OP_MUL:
        return a * b * rinv % BB_P
    if op == OP_ADD:
        return (a + b) % BB_P
    if op == OP_SUB:
        return (a - b) % BB_P
    if op in (OP_REDUCE64, OP_FROM_R64):
        return a * rinv % BB_P
    return a * BB_R % BB_P                      # TO_R64: v * (2^64 mod p) / 2^32


@functools.lru_cache(maxsize=None)
def bb_words():
    p = BB_P
    w = {0, 1, 2, p - 2, p - 1, (p - 1) // 2, (p + 1) // 2}
    for k in range(31):
        w |= {v for v in ((1 << k) - 1, 1 << k, (1 << k) + 1) if v < p}
    return sorted(w)


@functools.lru_cache(maxsize=None)
def bb_operands(op):
    p, w = BB_P, bb_words()
    rng = random.Random(7900 + op)
    word = lambda: rng.choice(w) if rng.random() < 0.5 else rng.randrange(p)
    if op in (OP_MUL, OP_ADD, OP_SUB):
        rows = list(itertools.product(w, w)) + [(word(), word()) for _ in range(N_RANDOM)]
    elif op == OP_REDUCE64:
        ks = [k for k in w if k]
        vals = [0, (p - 1) ** 2, 2 * (p - 1) ** 2, p * BB_R - 1] + [k << 32 for k in ks] + [(k << 32) - 1 for k in ks]
        # the two-term sums of the radix-4 butterfly, w1*cc + e1*d, at the largest words
        big = [p - 1, p - 2, (p + 1) // 2, (p - 1) // 2, 1 << 30, 1, 0]
        vals += [x * y + u * v for x, y, u, v in itertools.product(big, repeat=4)]
        vals += [word() * word() + word() * word() for _ in range(N_RANDOM // 2)] + [rng.randrange(p * BB_R) for _ in range(N_RANDOM // 2)]
        rows = [(v, None) for v in vals]
    else:                       # FROM_R64: a u64 below p; TO_R64: a word below p
        rows = [(v, None) for v in w] + [(word(), None) for _ in range(N_RANDOM)]
    assert all(v < (p * BB_R if op == OP_REDUCE64 else p) for r in rows for v in r if v is not None)
    return [r[0] for r in rows], ([r[1] for r in rows] if op in TWO_OPERANDS else None)


@functools.lru_cache(maxsize=None)
def bb_expected(op):
    a, b = bb_operands(op)
    return [bb_op(op, x, b[i] if b else None) for i, x in enumerate(a)]
