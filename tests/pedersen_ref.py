"""Big-integer restatement of the Starknet Pedersen hash over the Stark curve (crypto/src/hash/pedersen/mod.rs,
PedersenStarkCurve::hash) and of the 2-to-1 Merkle tree over leaf values built on it (utils.rs:24-71 node layout).
Independent of the library: the four lookup tables are generated here again from StarkWare's five published points.
Values are canonical Python integers, points are affine pairs or None for the point at infinity; to_elems / from_elems
convert to the library's boundary layout (4 x u64, most significant limb first, Montgomery form)."""
from tests.poseidon_ref import P, R, R_INV, bitrev, from_elems, raw_ints, to_elems  # noqa: F401  (the same field and layout)

A = 1
B = 0x6F21413EFBE40DE150E596D72F7A8C5609AD26C15C915C1F4CDFCB99CEE9E89
P0 = (0x049ee3eba8c1600700ee1b87eb599f16716b0b1022947733551fde4050ca6804, 0x03ca0cfe4b3bc6ddf346d49d06ea0ed34e621062c0e056c1d0405d266e10268a)
P1 = (0x0234287dcbaffe7f969c748655fca9e58fa8120b6d56eb0c1080d17957ebe47b, 0x03b056f100f96fb21e889527d41f4e39940135dd7a6c94cc6ed0268ee89e5615)
P2 = (0x04fa56f376c83db33f9dab2656558f3399099ec1de5e3018b7a6932dba8aa378, 0x03fa0984c931c9e38113e0c0e47e4401562761f92a7a23b45168f4e80ff5b54d)
P3 = (0x04ba4cc166be8dec764910f75b45f74b40c690c74709e90f3aa372f0bd2d6997, 0x0040301cf5c1751f4b971e46c4ede85fcac5c59a5ce5ae7c48151f27b24b219c)
P4 = (0x054302dcb0e6cc1c6e44cca8f61a63bb2ca65048d53fb325d36ff12c49a58202, 0x01b77b3e37d13504b348046268d8ae25ce98ad783c25561a879dcc77e99c2426)
LOW_CHUNKS, TABLE_SIZE = 62, 15                      # 62 nibbles of the low 248 bits, 15 non-zero values of a nibble
N_LOW, N_POINTS = LOW_CHUNKS * TABLE_SIZE, 1890      # 930 entries of T1 (T3), 930 + 15 + 930 + 15 in all


def on_curve(pt):
    return pt is None or (pt[1] * pt[1] - (pt[0] ** 3 + A * pt[0] + B)) % P == 0


def neg(pt):
    return None if pt is None else (pt[0], -pt[1] % P)


def add(p, q):
    """affine addition, every case: infinity, doubling, opposite points"""
    if p is None:
        return q
    if q is None:
        return p
    if p[0] == q[0]:
        if (p[1] + q[1]) % P == 0:
            return None
        lam = (3 * p[0] * p[0] + A) * pow(2 * p[1], -1, P) % P
    else:
        lam = (q[1] - p[1]) * pow(q[0] - p[0], -1, P) % P
    x = (lam * lam - p[0] - q[0]) % P
    return x, (lam * (p[0] - x) - p[1]) % P


def _table(base, chunks):
    """k * 2^(4 i) * base for i < chunks, k = 1 .. 15, entry 15 i + k - 1"""
    out = []
    for _ in range(chunks):
        acc = base
        for _ in range(TABLE_SIZE):
            out.append(acc)
            acc = add(acc, base)
        base = acc   # 16 * base
    return out


_TABLES = None


def tables():
    """T1 || T2 || T3 || T4: 1 890 affine points"""
    global _TABLES
    if _TABLES is None:
        _TABLES = _table(P1, LOW_CHUNKS) + _table(P2, 1) + _table(P3, LOW_CHUNKS) + _table(P4, 1)
        assert len(_TABLES) == N_POINTS
    return _TABLES


# Jacobian accumulator (X, Y, Z), x = X / Z^2, y = Y / Z^3, for speed only: the hash adds about 117 table points
def _jac_add_affine(acc, q):
    X1, Y1, Z1 = acc
    if Z1 == 0:
        return q[0], q[1], 1
    zz = Z1 * Z1 % P
    h = (q[0] * zz - X1) % P
    r = (q[1] * zz * Z1 - Y1) % P
    if h == 0:
        s = add((X1 * pow(zz, -1, P) % P, Y1 * pow(zz * Z1, -1, P) % P), q)   # doubling or infinity: the affine law
        return (1, 1, 0) if s is None else (s[0], s[1], 1)
    hh = h * h % P
    hhh = h * hh % P
    v = X1 * hh % P
    X3 = (r * r - hhh - 2 * v) % P
    return X3, (r * (v - X3) - Y1 * hhh) % P, Z1 * h % P


def hash(x, y):
    """PedersenStarkCurve::hash of canonical integers x, y < p"""
    assert 0 <= x < P and 0 <= y < P
    t = tables()
    acc = (P0[0], P0[1], 1)
    for v, off in ((x, 0), (y, N_LOW + TABLE_SIZE)):
        for i in range(LOW_CHUNKS + 1):   # chunk 62 is bits 248 .. 251: T2 (T4) follows T1 (T3) directly
            k = (v >> (4 * i)) & 15
            if k:
                acc = _jac_add_affine(acc, t[off + TABLE_SIZE * i + k - 1])
    return acc[0] * pow(acc[2] * acc[2], -1, P) % P


def tree_nodes(leaves):
    """nodes of the tree over the leaf values (a power of two of them): inner nodes root first, then the leaves"""
    n = len(leaves)
    assert n and n & (n - 1) == 0
    nodes = [0] * (n - 1) + list(leaves)
    for k in range(n - 2, -1, -1):
        nodes[k] = hash(nodes[2 * k + 1], nodes[2 * k + 2])
    return nodes


def commit_leaves(leaves, bit_reverse):
    """MerkleTree with hash_new_parent = PedersenStarkCurve::hash and identity leaves"""
    n = len(leaves)
    bits = n.bit_length() - 1
    return tree_nodes([leaves[bitrev(i, bits) if bit_reverse else i] for i in range(n)])


# ---- boundary layout of points: (x, y) as two elements, (0, 0) for the point at infinity
def points_to_elems(points):
    return to_elems([c for pt in points for c in (pt if pt is not None else (0, 0))]).reshape(len(points), 2, 4)


def points_from_elems(elems):
    v = from_elems(elems)
    return [None if (v[2 * i], v[2 * i + 1]) == (0, 0) else (v[2 * i], v[2 * i + 1]) for i in range(len(v) // 2)]
