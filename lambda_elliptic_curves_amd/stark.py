"""The STARK prover's DEEP composition polynomial (compute_deep_composition_poly / compute_trace_term,
provers/stark/src/prover.rs:643-714, 720-747) on the device, between round 3 and fri::commit_phase (:575-594):

    deep = sum_i gamma'_i (H_i - H_i(z^P)) / (X - z^P)  +  sum_j sum_r gamma_{j,r} (t_j - y_{j,r}) / (X - g^r z)

over Stark252 or BLS12-381 Fr.  Elements are as stored (Montgomery form, 4 x uint64, MS limb first).  The evaluations the
reference subtracts are not taken: they change only coefficient 0, which no quotient coefficient reads.  Scalars (z, g,
gamma) are host values; their few products are done here in Python integers on the stored limbs."""
import numpy as np

from . import _lib as L
from . import poly

MODULI = {
    L.FIELD_STARK252: (1 << 251) + 17 * (1 << 192) + 1,
    L.FIELD_BLS12_381_FR: 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001,
}


def _int(e):
    w = np.ascontiguousarray(e, dtype=np.uint64).reshape(-1)[:4]
    return (int(w[0]) << 192) | (int(w[1]) << 128) | (int(w[2]) << 64) | int(w[3])


def _limbs(v):
    return [(v >> s) & 0xffffffffffffffff for s in (192, 128, 64, 0)]


def deep_terms(field, n_trace_polys, n_parts, n_frame_rows, z, primitive_root, gamma):
    """The points and the weight matrix of the DEEP composition polynomial, for lw_stark_deep_composition:
    polynomials t_0 .. t_{C-1}, H_0 .. H_{P-1} (K = C + P rows), points g^0 z .. g^(T-1) z, z^P (M = T + 1 columns),
    T = n_frame_rows = transition_offsets.len() * STEP_SIZE.
    Row r of the frame is divided at g^r z with r the enumeration index, as compute_trace_term does (prover.rs:739).
    Weights are the powers 1, gamma, gamma^2, ... in the reference's order (prover.rs:559-572): the first C * T go to the
    trace terms in runs of T per column, the next P to the composition parts; every other entry is zero.
    -> (points (M, 4), weights (K, M, 4)) uint64, stored form."""
    p = MODULI[field.field]
    r_inv = pow(1 << 256, -1, p)
    mul = lambda a, b: a * b * r_inv % p          # the product of two stored values, stored
    one = (1 << 256) % p
    Z, G, GA = _int(z), _int(primitive_root), _int(gamma)
    C_, P_, T = int(n_trace_polys), int(n_parts), int(n_frame_rows)
    pts, gr = [], one
    for _ in range(T):
        pts.append(mul(gr, Z))
        gr = mul(gr, G)
    zp = one
    for _ in range(P_):
        zp = mul(zp, Z)
    pts.append(zp)
    w = [[0] * (T + 1) for _ in range(C_ + P_)]
    g = one
    for j in range(C_):
        for r in range(T):
            w[j][r] = g
            g = mul(g, GA)
    for i in range(P_):
        w[C_ + i][T] = g
        g = mul(g, GA)
    points = np.array([_limbs(v) for v in pts], dtype=np.uint64).reshape(T + 1, 4)
    weights = np.array([[_limbs(v) for v in row] for row in w], dtype=np.uint64).reshape(C_ + P_, T + 1, 4)
    return points, weights


def deep_composition_poly_device(field, t_trace_polys, trace_lens, t_parts, part_lens, z, primitive_root, n_frame_rows, gamma,
                                 t_out, stream=None):
    """compute_deep_composition_poly on device-resident polynomials into t_out (longest length - 1 elements), which
    merkle.fri_commit_phase_device takes as it is.  -> (stripped length, trace values (C, T, 4) with [j, r] = t_j(g^r z),
    composition part values (P, 4) = H_i(z^P)): round 3's out-of-domain tables at the points the division uses."""
    C_, P_, T = len(t_trace_polys), len(t_parts), int(n_frame_rows)
    points, weights = deep_terms(field, C_, P_, T, z, primitive_root, gamma)
    n, ev = poly.deep_composition_device(field, list(t_trace_polys) + list(t_parts), list(trace_lens) + list(part_lens), points,
                                         weights, t_out, stream=stream)
    return n, ev[:C_, :T].copy(), ev[C_:, T].copy()


# ---- round 4 after fri::commit_phase (provers/stark/src/prover.rs:596-617): grinding and the query openings

def grinding_window(grinding_factor):
    """Candidates per launch of the grinding search (lw_stark_grinding_window)."""
    return int(L.lib().lw_stark_grinding_window(int(grinding_factor)))


def grinding_nonce(seed, grinding_factor, first=0, last=2**64 - 1, stream=None):
    """grinding::generate_nonce (provers/stark/src/grinding.rs:40-53) on the device: the smallest nonce in [first, last] with
    u64_be(Keccak256(Keccak256(PREFIX || seed || grinding_factor) || nonce_be)[0..8]) < 2^(64 - grinding_factor), or None.
    2^64 - 1 is never a candidate, as in the reference's 0..u64::MAX: last = 2^64 - 1 means 2^64 - 2, and the range
    [2^64 - 1, 2^64 - 1] gives None.
    stream: a HIP stream handle (lw_stark_grinding_nonce_device); None: the library's own stream."""
    import ctypes as C
    from .errors import check
    seed = bytes(seed)
    if len(seed) != 32:
        from .errors import InputError
        raise InputError(f"the seed is {len(seed)} bytes, not 32")
    if not (0 <= int(first) < 2**64 and 0 <= int(last) < 2**64):
        from .errors import InputError
        raise InputError("nonces are 64-bit")
    buf = (C.c_uint8 * 32).from_buffer_copy(seed)
    nonce, found = C.c_uint64(0), C.c_int(0)
    if stream is None:
        check(L.lib().lw_stark_grinding_nonce(buf, int(grinding_factor), int(first), int(last), C.byref(nonce), C.byref(found)))
    else:
        check(L.lib().lw_stark_grinding_nonce_device(buf, int(grinding_factor), int(first), int(last), C.byref(nonce), C.byref(found),
                                                     C.c_void_p(stream)))
    return int(nonce.value) if found.value else None


def fri_query_phase_device(field, layers, iotas, stream=None):
    """fri::query_phase (provers/stark/src/fri/mod.rs:77-113) over the layers merkle.fri_commit_phase_device returned,
    [(t_evaluation, t_nodes, root, domain_size)], all resident.  -> per iota (layers_evaluations_sym, layers_auth_paths):
    the reference's FriDecommitment, evaluations as (n_layers, 4) uint64 and one (log2(domain/2), 32) uint8 path per layer."""
    from . import merkle
    iotas = [int(x) for x in iotas]
    if not layers or not iotas:
        return [] if not layers else [(np.zeros((0, 4), np.uint64), []) for _ in iotas]
    trees = [merkle.Tree(field, t_nodes, int(domain).bit_length() - 1, t_columns=t_ev, n_cols=1, rows_per_leaf=2, bit_reverse=False)
             for (t_ev, t_nodes, _root, domain) in layers]
    pos = np.array([[iota >> (k + 1) for iota in iotas] for k in range(len(layers))], np.uint64)
    values, paths = merkle.open_trees_device(trees, pos, stream=stream)
    out = []
    for s, iota in enumerate(iotas):
        # the leaf holds evaluation[index & ~1], evaluation[index | 1] with index = iota >> k; the symmetric one is index ^ 1
        sym = np.stack([values[k][s, ((iota >> k) & 1) ^ 1, 0] for k in range(len(layers))])
        out.append((sym, [paths[k][s] for k in range(len(layers))]))
    return out


def open_deep_composition_poly_device(field, main, composition, iotas, aux=None, stream=None):
    """open_deep_composition_poly (provers/stark/src/prover.rs:822-860) on resident LDE columns and trees.
    main / aux: (t_columns, n_cols, log2_rows, t_nodes) as lw_stark_commit_columns_device committed them (one bit-reversed row
    per leaf, open_trace_polys :794-820); composition: the same tuple for the tree over pairs of consecutive bit-reversed
    rows (2^(log2_rows - 1) leaves, :398-420, open_composition_poly :752-789).
    -> per iota a dict tree name -> dict(evaluations, evaluations_sym (each (n_cols, 4) uint64), proof, proof_sym
    ((log2 leaves, 32) uint8)): the reference's PolynomialOpenings; for the composition tree proof_sym is proof."""
    from . import merkle
    iotas = [int(x) for x in iotas]
    names = ["main", "composition"] + (["aux"] if aux is not None else [])
    if not iotas:
        return []
    q = len(iotas)
    trace_pos = [2 * x for x in iotas] + [2 * x + 1 for x in iotas]          # 2 q positions: index, then index_sym
    comp_pos = iotas + iotas                                                  # padded to the same q (duplicates are legal)
    trees, pos = [], []
    for name, src in (("main", main), ("composition", composition), ("aux", aux)):
        if src is None:
            continue
        t_cols, n_cols, log2_rows, t_nodes = src
        trees.append(merkle.Tree(field, t_nodes, log2_rows, t_columns=t_cols, n_cols=n_cols,
                                 rows_per_leaf=2 if name == "composition" else 1, bit_reverse=True))
        pos.append(comp_pos if name == "composition" else trace_pos)
    values, paths = merkle.open_trees_device(trees, np.array(pos, np.uint64), stream=stream)
    out = []
    for s in range(q):
        entry = {}
        for k, name in enumerate(names):
            if name == "composition":   # the even / odd split of prover.rs:778-787
                entry[name] = dict(evaluations=values[k][s, 0], evaluations_sym=values[k][s, 1], proof=paths[k][s], proof_sym=paths[k][s])
            else:
                entry[name] = dict(evaluations=values[k][s, 0], evaluations_sym=values[k][q + s, 0], proof=paths[k][s],
                                   proof_sym=paths[k][q + s])
        out.append(entry)
    return out


# ---- round 2 (provers/stark/src/prover.rs:428-484): constraint evaluations, the parts of H and their commitment

def _boundary_table(boundary):
    """[(col, step, value, coeff)] -> lw_stark_boundary_t array; col indexes the column table (main, then auxiliary)."""
    tab = (L.StarkBoundary * max(1, len(boundary)))()
    for k, (col, step, value, coeff) in enumerate(boundary):
        tab[k].col, tab[k].step = int(col), int(step)
        tab[k].value[:] = [int(x) for x in np.asarray(value, np.uint64).reshape(4)]
        tab[k].coeff[:] = [int(x) for x in np.asarray(coeff, np.uint64).reshape(4)]
    return tab


def _transition_table(transitions):
    """[dict(period, offset, end_exemptions, exemptions_period (None / 0: none), periodic_exemptions_offset, coeff)], the
    TransitionConstraint accessors of constraints/transition.rs:24-82 -> lw_stark_transition_t array."""
    tab = (L.StarkTransition * max(1, len(transitions)))()
    for k, t in enumerate(transitions):
        tab[k].period, tab[k].offset = int(t.get("period", 1)), int(t.get("offset", 0))
        tab[k].end_exemptions = int(t.get("end_exemptions", 0))
        tab[k].exemptions_period = int(t.get("exemptions_period") or 0)
        tab[k].periodic_exemptions_offset = int(t.get("periodic_exemptions_offset") or 0)
        tab[k].coeff[:] = [int(x) for x in np.asarray(t["coeff"], np.uint64).reshape(4)]
    return tab


def constraint_evaluations_device(field, t_columns, log2_trace, log2_blowup, coset_offset, boundary, transitions, t_transition_evals,
                                  t_out=None, transition_stride_elems=0, stream=None):
    """ConstraintEvaluator::evaluate (constraints/evaluator.rs:33-225) on resident LDE columns: t_columns is a list of
    tensors, one natural-order column of N = 2^(log2_trace + log2_blowup) elements each (main columns, then auxiliary);
    row c of t_transition_evals is compute_transition's value of constraint c at every LDE row, written by the caller.
    -> t_out (N, 4), the evaluations of the composition polynomial on the LDE coset."""
    import ctypes as C
    import torch
    from .errors import check
    n_lde = 1 << (int(log2_trace) + int(log2_blowup))
    ptrs = (C.c_void_p * max(1, len(t_columns)))(*[t.data_ptr() for t in t_columns])
    off = np.ascontiguousarray(coset_offset, dtype=np.uint64).reshape(4)
    dev = t_columns[0].device if len(t_columns) else t_transition_evals.device
    if t_out is None:
        t_out = torch.empty((n_lde, 4), dtype=torch.int64, device=dev)
    check(L.lib().lw_stark_constraint_evaluations_device(
        field.field, ptrs, len(t_columns), int(log2_trace), int(log2_blowup), off.ctypes.data_as(C.c_void_p),
        _boundary_table(boundary), len(boundary), _transition_table(transitions), len(transitions),
        C.c_void_p(t_transition_evals.data_ptr()) if t_transition_evals is not None else None, int(transition_stride_elems),
        C.c_void_p(t_out.data_ptr()), poly._stream(stream)))
    return t_out


def part_block_len(log2_lde, n_parts):
    """next_power_of_two(ceil(N / P)): the zero-padded block a part of H is stored in."""
    per = -(-(1 << int(log2_lde)) // int(n_parts))
    return 1 << (per - 1).bit_length()


def composition_parts_device(field, t_evals, log2_lde, coset_offset, n_parts, lde=True, lens=True, stream=None):
    """interpolate_offset_fft, break_in_parts (math/src/polynomial/mod.rs:289-302) and the LDE of every part.
    -> (t_parts_coeffs (P, L, 4), part_lens (stripped, None when lens=False: nothing is waited for), t_parts_lde (P, N, 4) or None)."""
    import ctypes as C
    import torch
    from .errors import check
    P, n_lde = int(n_parts), 1 << int(log2_lde)
    off = np.ascontiguousarray(coset_offset, dtype=np.uint64).reshape(4)
    t_coeffs = torch.empty((max(P, 1), part_block_len(log2_lde, max(P, 1)), 4), dtype=torch.int64, device=t_evals.device)
    t_lde = torch.empty((max(P, 1), n_lde, 4), dtype=torch.int64, device=t_evals.device) if lde else None
    ln = (C.c_size_t * max(1, P))()
    check(L.lib().lw_stark_composition_parts_device(field.field, C.c_void_p(t_evals.data_ptr()), int(log2_lde), off.ctypes.data_as(C.c_void_p),
                                                    P, C.c_void_p(t_coeffs.data_ptr()), C.c_void_p(t_lde.data_ptr()) if lde else None,
                                                    ln if lens else None, poly._stream(stream)))
    return t_coeffs, ([int(x) for x in ln] if lens else None), t_lde


def round2_device(field, t_columns, log2_trace, log2_blowup, coset_offset, boundary, transitions, t_transition_evals, n_parts,
                  transition_stride_elems=0, stream=None):
    """round_2_compute_composition_polynomial (provers/stark/src/prover.rs:428-484) on resident data.
    -> (t_parts_coeffs: the P coefficient blocks (views of one tensor), part_lens, t_parts_lde (P, N, 4), t_nodes, root):
    deep_composition_poly_device takes the first two as t_parts / part_lens, open_deep_composition_poly_device
    (t_parts_lde, P, log2_lde, t_nodes) as its composition tuple."""
    import torch
    from . import merkle
    log2_lde = int(log2_trace) + int(log2_blowup)
    t_ev = constraint_evaluations_device(field, t_columns, log2_trace, log2_blowup, coset_offset, boundary, transitions, t_transition_evals,
                                         transition_stride_elems=transition_stride_elems, stream=stream)
    t_coeffs, lens, t_lde = composition_parts_device(field, t_ev, log2_lde, coset_offset, n_parts, stream=stream)
    t_nodes = torch.empty((((1 << log2_lde) - 1) * 4,), dtype=torch.int64, device=t_ev.device)
    root = merkle.commit_composition_device(field, t_lde, n_parts, log2_lde, t_nodes, stream=stream)
    return [t_coeffs[j] for j in range(int(n_parts))], lens, t_lde, t_nodes, root


def round2(field, columns, log2_trace, log2_blowup, coset_offset, boundary, transitions, transition_evals, n_parts,
           return_nodes=False, return_lde=False):
    """round2_device on host arrays (lw_stark_round2): columns (n_cols, N, 4), transition_evals (n_transitions, N, 4).
    -> (parts_coeffs (P, L, 4), part_lens, root[, nodes (N - 1, 32)][, parts_lde (P, N, 4)])"""
    import ctypes as C
    from .errors import check
    log2_lde = int(log2_trace) + int(log2_blowup)
    n_lde, P = 1 << log2_lde, int(n_parts)
    cols = np.ascontiguousarray(columns, dtype=np.uint64).reshape(-1, n_lde, 4)
    tev = np.ascontiguousarray(transition_evals, dtype=np.uint64).reshape(-1, n_lde, 4)
    off = np.ascontiguousarray(coset_offset, dtype=np.uint64).reshape(4)
    coeffs = np.zeros((max(P, 1), part_block_len(log2_lde, max(P, 1)), 4), np.uint64)
    ln = (C.c_size_t * max(1, P))()
    root = np.zeros(32, np.uint8)
    nodes = np.zeros((n_lde - 1, 32), np.uint8) if return_nodes else None
    lde = np.zeros((max(P, 1), n_lde, 4), np.uint64) if return_lde else None
    vp = lambda x: x.ctypes.data_as(C.c_void_p) if x is not None else None
    check(L.lib().lw_stark_round2(field.field, vp(cols), cols.shape[0], int(log2_trace), int(log2_blowup), vp(off),
                                  _boundary_table(boundary), len(boundary), _transition_table(transitions), len(transitions), vp(tev),
                                  P, vp(coeffs), ln, vp(root), vp(nodes), vp(lde)))
    out = (coeffs, [int(x) for x in ln], root.tobytes())
    if return_nodes:
        out += (nodes,)
    if return_lde:
        out += (lde,)
    return out


# ---- transition constraints from an AIR given as data (csrc/stark_air.hip): compute_transition as a straight-line program

class Expr:
    """A polynomial expression over frame cells and constants: cell() and const() are the leaves, + - * and unary - build
    the tree.  Two uses of the same Python object are one sub-expression, computed once."""
    __slots__ = ("kind", "a", "b")

    def __init__(self, kind, a=None, b=None):
        self.kind, self.a, self.b = kind, a, b

    def _bin(self, kind, other):
        return Expr(kind, self, other) if isinstance(other, Expr) else NotImplemented

    def __add__(self, o):
        return self._bin("add", o)

    def __sub__(self, o):
        return self._bin("sub", o)

    def __mul__(self, o):
        return self._bin("mul", o)

    def __neg__(self):
        return Expr("neg", self)

    @property
    def is_leaf(self):
        return self.kind in ("cell", "const", "xcell", "xconst")


def cell(col, row=0):
    """column `col` of the frame at trace-row offset `row` (offset * STEP_SIZE + row in the step)"""
    col, row = int(col), int(row)
    if not (0 <= col < 1 << 16 and 0 <= row < 1 << 32):
        from .errors import InputError
        raise InputError(f"cell({col}, {row})")
    return Expr("cell", col, row)


def const(k):
    """consts[k] of the call: a challenge or a literal of the AIR"""
    k = int(k)
    if not 0 <= k < L.AIR_MAX_CONSTS:
        from .errors import InputError
        raise InputError(f"const({k}): a program has at most {L.AIR_MAX_CONSTS} constants")
    return Expr("const", k)


def xcell(col, row=0):
    """auxiliary column `col` of the frame at trace-row offset `row`, an element of the extension: the _rap_ entry points of
    goldilocks_ext and babybear_ext only"""
    col, row = int(col), int(row)
    if not (0 <= col < 1 << 16 and 0 <= row < 1 << 32):
        from .errors import InputError
        raise InputError(f"xcell({col}, {row})")
    return Expr("xcell", col, row)


def xconst(k):
    """xconsts[k] of the call, an element of the extension: a challenge of a randomized AIR"""
    k = int(k)
    if not 0 <= k < L.AIR_MAX_CONSTS:
        from .errors import InputError
        raise InputError(f"xconst({k}): a program has at most {L.AIR_MAX_CONSTS} extension constants")
    return Expr("xconst", k)


AIR_OP_DTYPE = np.dtype([("op", "u1"), ("src", "u1"), ("index", "<u2"), ("row", "<u4")])   # lw_stark_air_op_t


class AirProgram:
    """ops: (n_ops,) AIR_OP_DTYPE; n_transitions constraints; n_tmps temporaries used; n_consts and n_cols: one more than
    the highest constant and column the program reads, n_xconsts and n_xcols the same of the extension's constants and the
    auxiliary columns; n_mul: its MUL count."""

    def __init__(self, ops, n_transitions):
        self.ops = np.ascontiguousarray(ops, dtype=AIR_OP_DTYPE).reshape(-1)
        self.n_transitions = int(n_transitions)
        op, src, idx = self.ops["op"], self.ops["src"], self.ops["index"].astype(np.int64)
        reads = op <= L.AIR_MUL
        top = lambda mask: int(idx[mask].max()) + 1 if mask.any() else 0
        self.n_tmps = top(op == L.AIR_STORE)
        self.n_consts = top(reads & (src == L.AIR_CONST))
        self.n_cols = top(reads & (src == L.AIR_CELL))
        self.n_xconsts = top(reads & (src == L.AIR_XCONST))
        self.n_xcols = top(reads & (src == L.AIR_XCELL))
        self.n_mul = int((op == L.AIR_MUL).sum())

    def __len__(self):
        return self.ops.shape[0]


def compile_transitions(exprs):
    """[expr_0, expr_1, ...] -> AirProgram emitting T_c = expr_c.  A leaf operand is used directly; a compound right
    operand is computed first and kept in a temporary while the left one is computed; a compound sub-expression used more
    than once (the same object) is computed at its first use and kept in a temporary until its last.  More than
    LW_STARK_AIR_MAX_TMPS temporaries alive at once, or more than LW_STARK_AIR_MAX_OPS ops: errors.InputError."""
    from .errors import InputError
    exprs = list(exprs)
    uses, seen, stack = {}, set(), list(exprs)
    for e in exprs:
        if not isinstance(e, Expr):
            raise InputError(f"not an expression: {e!r}")
        uses[id(e)] = uses.get(id(e), 0) + 1
    while stack:                                   # one visit per node, one count per edge
        e = stack.pop()
        if id(e) in seen or e.is_leaf:
            continue
        seen.add(id(e))
        for ch in (e.a, e.b):
            if isinstance(ch, Expr):
                uses[id(ch)] = uses.get(id(ch), 0) + 1
                stack.append(ch)
    ops, free, kept = [], list(range(L.AIR_MAX_TMPS)), {}      # kept: id -> slot of a shared sub-expression already computed
    OPC = {"add": L.AIR_ADD, "sub": L.AIR_SUB, "mul": L.AIR_MUL}

    def emit(op, src=0, index=0, row=0):
        if len(ops) >= L.AIR_MAX_OPS:
            raise InputError(f"the program needs more than {L.AIR_MAX_OPS} ops")
        ops.append((op, src, index, row))

    def take():
        if not free:
            raise InputError(f"the expressions need more than {L.AIR_MAX_TMPS} temporaries at once")
        return free.pop(0)

    def give(slot):
        free.append(slot)
        free.sort()

    def operand(e):
        """(src, index, row) of an expression that needs no code: a leaf, or a shared one already in its temporary"""
        if e.kind == "cell":
            return (L.AIR_CELL, e.a, e.b)
        if e.kind == "const":
            return (L.AIR_CONST, e.a, 0)
        if e.kind == "xcell":
            return (L.AIR_XCELL, e.a, e.b)
        if e.kind == "xconst":
            return (L.AIR_XCONST, e.a, 0)
        if id(e) in kept:
            return (L.AIR_TMP, kept[id(e)], 0)
        return None

    def used(e):
        """one use of a kept sub-expression is over"""
        if id(e) in kept:
            uses[id(e)] -= 1
            if uses[id(e)] == 0:
                give(kept.pop(id(e)))

    def gen(e):
        """acc = e; whoever consumes acc calls used(e) afterwards"""
        direct = operand(e)
        if direct is not None:
            emit(L.AIR_LOAD, *direct)
            return
        if e.kind == "neg":
            gen(e.a)
            emit(L.AIR_NEG)
            used(e.a)
        elif operand(e.b) is not None:
            gen(e.a)
            emit(OPC[e.kind], *operand(e.b))
            used(e.a)
            used(e.b)
        else:
            gen(e.b)
            shared = id(e.b) in kept                # gen stored it in its own slot
            slot = kept[id(e.b)] if shared else take()
            if not shared:
                emit(L.AIR_STORE, 0, slot)
            gen(e.a)
            emit(OPC[e.kind], L.AIR_TMP, slot, 0)
            used(e.a)
            if shared:
                used(e.b)
            else:
                give(slot)
        if uses.get(id(e), 0) > 1:                  # the first of several uses: keep it
            kept[id(e)] = take()
            emit(L.AIR_STORE, 0, kept[id(e)])

    import sys
    limit = sys.getrecursionlimit()
    sys.setrecursionlimit(max(limit, 3 * L.AIR_MAX_OPS + 1000))
    try:
        for c, e in enumerate(exprs):
            if c >= 1 << 16:
                raise InputError("more than 65536 constraints")
            gen(e)
            emit(L.AIR_EMIT, 0, c)
            used(e)
    finally:
        sys.setrecursionlimit(limit)
    return AirProgram(np.array(ops, dtype=AIR_OP_DTYPE) if ops else np.zeros(0, AIR_OP_DTYPE), len(exprs))


def _air_args(program, consts, col_log2_len, n_cols, n_lde):
    """the program, the constants and the column lengths as the C calls take them (+ the objects that own the memory)"""
    import ctypes as C
    from .errors import LengthMismatch
    ops = np.ascontiguousarray(program.ops, dtype=AIR_OP_DTYPE)
    cs = np.ascontiguousarray(consts if consts is not None else np.zeros((0, 4), np.uint64), dtype=np.uint64).reshape(-1, 4)
    if cs.shape[0] < program.n_consts:
        raise LengthMismatch(f"{cs.shape[0]} constants for a program that reads constant {program.n_consts - 1}")
    if n_cols < program.n_cols:
        raise LengthMismatch(f"{n_cols} columns for a program that reads column {program.n_cols - 1}")
    lens = None
    if col_log2_len is not None:
        lens = np.ascontiguousarray([int(x) for x in col_log2_len], dtype=np.uint32)
        if lens.shape[0] != n_cols:
            raise LengthMismatch(f"{lens.shape[0]} column lengths for {n_cols} columns")
    col_elems = [n_lde if lens is None else 1 << int(x) for x in (lens if lens is not None else range(n_cols))]
    return (ops, cs, lens, col_elems,
            ops.ctypes.data_as(C.POINTER(L.StarkAirOp)) if ops.shape[0] else None, L.host_ptr(cs),
            lens.ctypes.data_as(C.POINTER(C.c_uint32)) if lens is not None else None)


def transition_evaluations_device(field, program, consts, t_columns, log2_trace, log2_blowup, col_log2_len=None, t_out=None, stream=None):
    """The AIR's compute_transition at every LDE row (lw_stark_transition_evaluations_device): t_columns is a list of
    resident columns, N = 2^(log2_trace + log2_blowup) elements each or 2^col_log2_len[c] for a short (periodic) one;
    consts (n_consts, 4) host elements.  -> t_out (n_transitions, stride, 4) with row c = T_c in its first N elements, as
    constraint_evaluations_device reads it with transition_stride_elems = stride.  A t_out of the caller's may have a
    stride above N (the gap is not written); one too short for n_transitions rows of N: errors.LengthMismatch.
    Enqueues on the stream and returns."""
    import ctypes as C
    import torch
    from .errors import LengthMismatch, check
    n_lde = 1 << (int(log2_trace) + int(log2_blowup))
    ops, cs, lens, col_elems, p_ops, p_cs, p_lens = _air_args(program, consts, col_log2_len, len(t_columns), n_lde)
    for c, (t, want) in enumerate(zip(t_columns, col_elems)):
        if t.numel() < want * 4:
            raise LengthMismatch(f"column {c}: {t.numel() // 4} elements, {want} needed")
    T = program.n_transitions
    if t_out is None:
        dev = t_columns[0].device if len(t_columns) else "cuda"
        t_out = torch.empty((max(T, 1), n_lde, 4), dtype=torch.int64, device=dev)
    stride = int(t_out.shape[1]) if t_out.dim() == 3 else n_lde
    if not t_out.is_contiguous() or (T and (stride < n_lde or t_out.numel() < ((T - 1) * stride + n_lde) * 4)):
        raise LengthMismatch(f"t_out of shape {tuple(t_out.shape)} for {T} rows of {n_lde} elements")
    ptrs = (C.c_void_p * max(1, len(t_columns)))(*[t.data_ptr() for t in t_columns])
    check(L.lib().lw_stark_transition_evaluations_device(field.field, p_ops, ops.shape[0], p_cs, cs.shape[0], ptrs, p_lens, len(t_columns),
                                                         int(log2_trace), int(log2_blowup), T, C.c_void_p(t_out.data_ptr()), stride,
                                                         poly._stream(stream)))
    return t_out


def transition_evaluations(field, program, consts, columns, log2_trace, log2_blowup, col_log2_len=None):
    """transition_evaluations_device on host arrays (lw_stark_transition_evaluations): columns is a list of (len, 4)
    arrays (or one (n_cols, N, 4) array).  -> (n_transitions, N, 4) uint64"""
    from .errors import LengthMismatch, check
    n_lde = 1 << (int(log2_trace) + int(log2_blowup))
    cols = [np.ascontiguousarray(c, dtype=np.uint64).reshape(-1, 4) for c in columns]
    ops, cs, lens, col_elems, p_ops, p_cs, p_lens = _air_args(program, consts, col_log2_len, len(cols), n_lde)
    for c, (a, want) in enumerate(zip(cols, col_elems)):
        if a.shape[0] != want:
            raise LengthMismatch(f"column {c}: {a.shape[0]} elements, {want} expected")
    flat = np.concatenate(cols) if cols else np.zeros((0, 4), np.uint64)
    out = np.zeros((program.n_transitions, n_lde, 4), np.uint64)
    check(L.lib().lw_stark_transition_evaluations(field.field, p_ops, ops.shape[0], p_cs, cs.shape[0], L.host_ptr(flat), p_lens, len(cols),
                                                  int(log2_trace), int(log2_blowup), program.n_transitions, L.host_ptr(out)))
    return out


def round2_program_device(field, t_columns, log2_trace, log2_blowup, coset_offset, boundary, transitions, program, consts, n_parts,
                          col_log2_len=None, stream=None):
    """round2_device with the transition evaluations computed on the device from the AIR's program: the T table never
    leaves the device.  t_columns may end in short (periodic) columns, which no boundary constraint refers to.
    -> what round2_device returns."""
    t_tev = transition_evaluations_device(field, program, consts, t_columns, log2_trace, log2_blowup, col_log2_len=col_log2_len, stream=stream)
    return round2_device(field, t_columns, log2_trace, log2_blowup, coset_offset, boundary, transitions, t_tev, n_parts, stream=stream)
