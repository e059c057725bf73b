"""Restatement of the PLONK prover's rounds 1-3 (provers/plonk/src/prover.rs:311-535, without the commitments) for any
n, field, witness, permutation, public input and blinders, in Python integers and literally as the reference writes
them: one division per row in round 2, seventeen coset evaluations and a batch inversion in round 3, polynomial
arithmetic for the blinding.  The transforms go through the CPU checker's evaluate_fft / interpolate_fft.  All values
are canonical integers mod the field's prime; polynomials are coefficient lists."""
import numpy as np

from oracle import bigint_def as D
from oracle import oracle as O


class Fld:
    def __init__(self, name, oid, p):
        self.name, self.oid, self.p = name, oid, p


STARK252 = Fld("stark252", O.F_STARK252, D.P_STARK252)
FR381 = Fld("fr381", O.F_FR381, D.P_FR381)
FIELDS = {"stark252": STARK252, "fr381": FR381}


# ---- integers <-> the reference's memory form ((len, 4) uint64, MS limb first, times 2^256)
def to_ints(a):
    a = np.ascontiguousarray(a, dtype=np.uint64).reshape(-1, 4)
    b = a.astype(">u8").tobytes()
    return [int.from_bytes(b[32 * i:32 * i + 32], "big") for i in range(a.shape[0])]


def to_arr(vals):
    if not len(vals):
        return np.zeros((0, 4), np.uint64)
    b = b"".join(int(v).to_bytes(32, "big") for v in vals)
    return np.frombuffer(b, dtype=">u8").astype(np.uint64).reshape(-1, 4)


def mont(f, vals):
    return to_arr([v * (1 << 256) % f.p for v in vals])


def unmont(f, a):
    ri = pow(1 << 256, -1, f.p)
    return [v * ri % f.p for v in to_ints(a)]


# ---- the polynomial operations the reference calls
def strip(f, c):
    c = list(c)
    while c and c[-1] % f.p == 0:
        c.pop()
    return c


def omega(f, n):
    """the primitive n-th root of unity the reference's domain is built from (n a power of two)"""
    return unmont(f, O.get_primitive_root_of_unity(f.oid, n.bit_length() - 1).reshape(1, 4))[0]


def interpolate_fft(f, evals):
    return unmont(f, O.interpolate_fft(f.oid, mont(f, evals)))


def evaluate_offset_fft(f, coeffs, domain_size, offset):
    return unmont(f, O.evaluate_fft(f.oid, mont(f, strip(f, coeffs)), 1, domain_size, mont(f, [offset])[0]))


def interpolate_offset_fft(f, evals, offset):
    return unmont(f, O.interpolate_fft(f.oid, mont(f, evals), mont(f, [offset])[0]))


def padd(f, a, b):
    out = [0] * max(len(a), len(b))
    for i, c in enumerate(a):
        out[i] = c
    for i, c in enumerate(b):
        out[i] = (out[i] + c) % f.p
    return out


def pmul(f, a, b):
    if not a or not b:
        return []
    out = [0] * (len(a) + len(b) - 1)
    for i, x in enumerate(a):
        if x:
            for j, y in enumerate(b):
                out[i + j] = (out[i + j] + x * y) % f.p
    return out


def padded(c, length):
    assert len(c) <= length, (len(c), length)
    return list(c) + [0] * (length - len(c))


def blind_polynomial(f, target, n, bs):
    """target + blinder * random_part with blinder = X^n - 1 (prover.rs:296-309)"""
    z_h = [f.p - 1] + [0] * (n - 1) + [1]
    return padd(f, target, pmul(f, z_h, strip(f, bs)))


# ---- the rounds
def round_1(f, n, witness, blinders=None):
    """witness: (a, b, c) lists of n values; blinders: six values or None -> [p_a, p_b, p_c], n + 2 coefficients each"""
    bs = list(blinders) if blinders is not None else [0] * 6
    return [padded(blind_polynomial(f, strip(f, interpolate_fft(f, w)), n, bs[2 * k:2 * k + 2]), n + 2) for k, w in enumerate(witness)]


def round_2(f, n, k1, witness, s_lagrange, beta, gamma, blinders=None):
    """-> (the n values z_i, p_z with n + 3 coefficients).  A zero denominator raises ValueError, as the reference's
    division panics."""
    p = f.p
    wa, wb, wc = witness
    s1, s2, s3 = s_lagrange
    w = omega(f, n)
    domain = [pow(w, i, p) for i in range(n)]
    k2 = k1 * k1 % p
    lp = lambda wv, eta: (wv + beta * eta + gamma) % p
    coefficients = [1]
    for i in range(n - 1):
        num = lp(wa[i], domain[i]) * lp(wb[i], domain[i] * k1 % p) * lp(wc[i], domain[i] * k2 % p) % p
        den = lp(wa[i], s1[i]) * lp(wb[i], s2[i]) * lp(wc[i], s3[i]) % p
        new_factor = num * pow(den, -1, p) % p
        coefficients.append(coefficients[-1] * new_factor % p)
    bs = list(blinders) if blinders is not None else [0] * 3
    p_z = blind_polynomial(f, strip(f, interpolate_fft(f, coefficients)), n, bs)
    return coefficients, padded(p_z, n + 3)


def round_3(f, n, k1, q_coeffs, s_coeffs, p_abc, p_z, public_input, beta, gamma, alpha, blinders=None):
    """q_coeffs: (ql, qr, qo, qm, qc), s_coeffs: (s1, s2, s3), p_abc: (p_a, p_b, p_c), all coefficient lists ->
    [t_lo, t_mid, t_hi], n + 3 coefficients each"""
    p = f.p
    ql, qr, qo, qm, qc = q_coeffs
    s1, s2, s3 = s_coeffs
    p_a, p_b, p_c = p_abc
    w = omega(f, n)
    domain = [pow(w, i, p) for i in range(n)]
    k2 = k1 * k1 % p
    zh = [p - 1] + [0] * (n - 1) + [1]
    z_x_omega = strip(f, [c * domain[i % n] % p for i, c in enumerate(strip(f, p_z))])
    l1 = interpolate_fft(f, [1] + [0] * (n - 1))
    p_pi = interpolate_fft(f, list(public_input) + [0] * (n - len(public_input)))
    degree = 4 * n
    ev = lambda c: evaluate_offset_fft(f, c, degree, k1)
    a_e, b_e, c_e = ev(p_a), ev(p_b), ev(p_c)
    ql_e, qr_e, qm_e, qo_e, qc_e, pi_e = ev(ql), ev(qr), ev(qm), ev(qo), ev(qc), ev(p_pi)
    x_e, z_e, zw_e = ev([0, 1]), ev(p_z), ev(z_x_omega)
    s1_e, s2_e, s3_e, l1_e = ev(s1), ev(s2), ev(s3), ev(l1)
    constraints = [(a * b * qm_ + a * ql_ + b * qr_ + c * qo_ + qc_ + pi) % p
                   for a, b, c, ql_, qr_, qm_, qo_, qc_, pi in zip(a_e, b_e, c_e, ql_e, qr_e, qm_e, qo_e, qc_e, pi_e)]
    f_e = [(a + x * beta + gamma) * (b + x * beta * k1 + gamma) * (c + x * beta * k2 + gamma) % p
           for a, b, c, x in zip(a_e, b_e, c_e, x_e)]
    g_e = [(a + u1 * beta + gamma) * (b + u2 * beta + gamma) * (c + u3 * beta + gamma) % p
           for a, b, c, u1, u2, u3 in zip(a_e, b_e, c_e, s1_e, s2_e, s3_e)]
    perm_1 = [(g * y - ff * z) % p for g, ff, z, y in zip(g_e, f_e, z_e, zw_e)]
    perm_2 = [(z - 1) * l % p for z, l in zip(z_e, l1_e)]
    p_e = [((p2 * alpha + p1) * alpha + co) % p for p2, p1, co in zip(perm_2, perm_1, constraints)]
    zh_e = [pow(v, -1, p) for v in ev(zh)]   # inplace_batch_inverse
    c_e2 = [a * b % p for a, b in zip(p_e, zh_e)]
    t = strip(f, interpolate_offset_fft(f, c_e2, k1))
    if len(t) < 3 * (n + 2):
        t = t + [0] * (3 * (n + 2) - len(t))
    t_lo, t_mid, t_hi = t[:n + 2], t[n + 2:2 * (n + 2)], t[2 * (n + 2):3 * (n + 2)]
    b_0, b_1 = blinders if blinders is not None else (0, 0)
    mono = lambda b: [0] * (n + 2) + [b]
    t_lo = padd(f, t_lo, mono(b_0))
    t_mid = padd(f, padd(f, t_mid, [(-b_0) % p]), mono(b_1))
    t_hi = padd(f, t_hi, [(-b_1) % p])
    return [padded(t_lo, n + 3), padded(t_mid, n + 3), padded(t_hi, n + 3)]


# ---- circuits
def reference_test_circuit():
    """test_common_preprocessed_input_1 / test_witness_1 (provers/plonk/src/test_utils/circuit_1.rs), with the challenges
    the reference's own tests hard-code (tests/plonk_kat.py)"""
    from tests import plonk_kat as K
    f, n, p = FR381, K.N, K.R
    w = omega(f, n)
    x, e = 2, 2
    y = x * e % p
    identity = [pow(w, row, p) * pow(K.K1, col, p) % p for col in range(3) for row in range(n)]
    permuted = [identity[K.PERMUTATION[i]] for i in range(3 * n)]
    s_lagrange = [permuted[:n], permuted[n:2 * n], permuted[2 * n:]]
    neg1 = p - 1
    q_lagrange = [[neg1, neg1, 0, 1], [0, 0, 0, neg1], [0, 0, neg1, 0], [0, 0, 1, 0], [0, 0, 0, 0]]   # ql qr qo qm qc
    return dict(field=f, n=n, k1=K.K1, witness=[[x, y, x, y], [x, x, e, y], [x, x, y, x]], s_lagrange=s_lagrange,
                q_coeffs=[interpolate_fft(f, c) for c in q_lagrange], s_coeffs=[interpolate_fft(f, c) for c in s_lagrange],
                public_input=[2, 4], beta=K.BETA, gamma=K.GAMMA, alpha=K.ALPHA)


def random_circuit(f, n, seed, n_pub=0):
    """Random witness, permutation values, selector and permutation polynomials: not a satisfiable circuit — the rounds
    are arithmetic on whatever they are given — so the quotient's dropped high coefficients are non-zero."""
    rng = np.random.default_rng(seed)
    rnd = lambda count: [int.from_bytes(rng.bytes(40), "big") % f.p for _ in range(count)]
    return dict(field=f, n=n, k1=7, witness=[rnd(n) for _ in range(3)], s_lagrange=[rnd(n) for _ in range(3)],
                q_coeffs=[rnd(n) for _ in range(5)], s_coeffs=[rnd(n) for _ in range(3)], public_input=rnd(n_pub),
                beta=rnd(1)[0], gamma=rnd(1)[0], alpha=rnd(1)[0])
