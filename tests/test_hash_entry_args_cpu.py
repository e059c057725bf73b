"""The argument checks of every lw_poseidon_*, lw_rpo_*, lw_pedersen_* and lw_monolith_* entry point, one fault at a time:
status and lw_hip_last_error() text of every refusal, and LW_OK for every call without work.  Every case is refused by
a check or has nothing to do, so no pointer is followed, no device is touched and the result is the same with and
without a GPU (the style of test_host_side_argument_checks_do_not_need_a_device)."""
import ctypes as C

import numpy as np

from lambda_elliptic_curves_amd import _lib

OK, BAD_ARG, ALLOC = _lib.OK, _lib.ERR_BAD_ARG, _lib.ERR_ALLOC
ALIGN = "device buffers must be 16-byte aligned"
NO_COLUMNS = "null buffer or no columns"
BIG = 2**36 + 1           # one above the count limit of every hash
LONG = 2**31 + 1          # one above the row length limit
WIDTH = lambda w: f"Monolith width {w}: 8, 12, 16, 20 or 24"
ROUNDS = lambda r: f"Monolith rounds {r}: 1 .. 15"
LEVEL = lambda v: f"bad RPO level {v}"

_mem = np.zeros(4096, np.uint8)   # never read or written: the calls below end before any pointer is followed
A = (_mem.ctypes.data + 15) & ~15
B, D, E = A + 256, A + 512, A + 768
vp, sz, u32, u64, i = C.c_void_p, C.c_size_t, C.c_uint32, C.c_uint64, C.c_int


def _library():
    L = C.CDLL(_lib.LIB_PATH)   # a handle of its own: plain ctypes arguments, no argtypes
    L.lw_hip_last_error.restype = C.c_char_p
    return L


def _entries(L):
    """name -> (f(dev, **overrides), the forms it has); every f has defaults that pass all checks"""
    def two(host, device):   # the host form and the _device form, which takes a stream last
        return lambda dev, *a: device(*a, None) if dev else host(*a)

    po_permute = two(L.lw_poseidon_permute, L.lw_poseidon_permute_device)
    po_hash = two(L.lw_poseidon_hash, L.lw_poseidon_hash_device)
    po_single = two(L.lw_poseidon_hash_single, L.lw_poseidon_hash_single_device)
    po_many = two(L.lw_poseidon_hash_many, L.lw_poseidon_hash_many_device)
    rpo_permute = two(L.lw_rpo_permute, L.lw_rpo_permute_device)
    pe_hash = two(L.lw_pedersen_hash, L.lw_pedersen_hash_device)
    mo_permute = two(L.lw_monolith_permute, L.lw_monolith_permute_device)
    mo_compress = two(L.lw_monolith_compress, L.lw_monolith_compress_device)
    BOTH, HOST, DEV = (False, True), (False,), (True,)

    def rows(host, device):   # (selector, rows, n_rows, row_len[, row_stride], out[, stream])
        def f(dev, sel=i(0), rows=A, n_rows=1, row_len=2, row_stride=0, out=B):
            if dev:
                return device(sel, vp(rows), sz(n_rows), sz(row_len), sz(row_stride), vp(out), None)
            return host(sel, vp(rows), sz(n_rows), sz(row_len), vp(out))
        return f

    def commit(host, device, lead, tail):   # lead: the selector in front (or none); tail: Poseidon's leaf mode behind bit_reverse
        def f(dev, sel=0, columns=A, n_cols=1, col_stride=0, log2n=3, mode=1, nodes=B, root=D):
            head = [lead(sel)] if lead else []
            if dev:
                return device(*head, vp(columns), u32(n_cols), u64(col_stride), u32(log2n), i(1), *([i(mode)] if tail else []), vp(nodes), vp(root), None)
            return host(*head, vp(columns), u32(n_cols), u32(log2n), i(1), *([i(mode)] if tail else []), vp(root), None)
        return f

    def pedersen_commit(dev, leaves=A, n_cols=1, log2n=3, nodes=B, root=D):
        if dev:
            return L.lw_pedersen_commit_leaves_device(vp(leaves), u32(n_cols), u32(log2n), i(1), vp(nodes), vp(root), None)
        return L.lw_pedersen_commit_leaves(vp(leaves), u32(n_cols), u32(log2n), i(1), vp(root), None)

    return {
        "poseidon_permute": (lambda dev, states=A, n=1, out=B: po_permute(dev, vp(states), sz(n), vp(out)), BOTH),
        "poseidon_hash": (lambda dev, x=A, y=B, n=1, out=D: po_hash(dev, vp(x), vp(y), sz(n), vp(out)), BOTH),
        "poseidon_hash_single": (lambda dev, x=A, n=1, out=B: po_single(dev, vp(x), sz(n), vp(out)), BOTH),
        "poseidon_hash_many": (lambda dev, rows=A, n_rows=1, row_len=2, out=B: po_many(dev, vp(rows), sz(n_rows), sz(row_len), vp(out)), BOTH),
        "poseidon_commit_columns": (commit(L.lw_poseidon_commit_columns, L.lw_poseidon_commit_columns_device, None, True), BOTH),
        "rpo_permute": (lambda dev, level=0, states=A, n=1, out=B: rpo_permute(dev, i(level), vp(states), sz(n), vp(out)), BOTH),
        "rpo_hash": (lambda dev, level=0, **kw: rows(L.lw_rpo_hash, L.lw_rpo_hash_device)(dev, i(level), **kw), BOTH),
        "rpo_commit_columns": (commit(L.lw_rpo_commit_columns, L.lw_rpo_commit_columns_device, i, False), BOTH),
        "pedersen_table": (lambda dev, out=A: L.lw_pedersen_table(vp(out)), HOST),
        "pedersen_hash": (lambda dev, x=A, y=B, n=1, out=D: pe_hash(dev, vp(x), vp(y), sz(n), vp(out)), BOTH),
        "pedersen_add_affine": (lambda dev, p=A, z=B, q=D, n=1, out=E: L.lw_pedersen_add_affine_device(vp(p), vp(z), vp(q), sz(n), vp(out), None), DEV),
        "pedersen_commit_leaves": (pedersen_commit, BOTH),
        "monolith_constants": (lambda dev, width=16, rounds=5, rc=A, mds=B: L.lw_monolith_constants(u32(width), u32(rounds), vp(rc), vp(mds)), HOST),
        "monolith_permute": (lambda dev, width=16, rounds=5, states=A, n=1, out=B: mo_permute(dev, u32(width), u32(rounds), vp(states), sz(n), vp(out)), BOTH),
        "monolith_layer": (lambda dev, width=16, rounds=5, layer=0, states=A, n=1, out=B:
                           L.lw_monolith_layer_device(u32(width), u32(rounds), i(layer), vp(states), sz(n), vp(out), None), DEV),
        "monolith_hash": (lambda dev, rounds=5, **kw: rows(L.lw_monolith_hash, L.lw_monolith_hash_device)(dev, u32(rounds), **kw), BOTH),
        "monolith_compress": (lambda dev, rounds=5, left=A, right=B, n=1, out=D: mo_compress(dev, u32(rounds), vp(left), vp(right), sz(n), vp(out)), BOTH),
        "monolith_commit_columns": (lambda dev, rounds=5, **kw: commit(L.lw_monolith_commit_columns, L.lw_monolith_commit_columns_device, u32, False)(dev, sel=rounds, **kw), BOTH),
    }


def _cases(L):
    """(label, call, status, text) for every fault; text None: the status alone counts"""
    entries = _entries(L)
    out = []

    def add(name, status, text, forms=None, **overrides):
        f, has = entries[name]
        for dev in has if forms is None else forms:
            label = "%s%s %s" % (name, "_device" if dev else "", " ".join(f"{k}={v}" for k, v in overrides.items()))
            out.append((label, lambda f=f, dev=dev: f(dev, **overrides), status, text))

    def flat(name, bufs, noun, count="n"):   # the checks every batched entry shares
        for b in bufs:
            add(name, BAD_ARG, "null buffer", **{b: 0})
            add(name, BAD_ARG, ALIGN, forms=[d for d in entries[name][1] if d], **{b: A + 8})
        add(name, ALLOC, f"{BIG} {noun} inputs", **{count: BIG})
        add(name, ALLOC, None, **{count: BIG, bufs[0]: 0})   # two faults: the count is looked at first
        add(name, OK, None, **{count: 0}, **{b: 0 for b in bufs})

    def row_shape(name, noun, unit, strided):
        flat(name, ["rows", "out"], noun, count="n_rows")
        add(name, ALLOC, f"1 rows of {LONG} {unit}", row_len=LONG)
        add(name, ALLOC, f"{2**35 + 1} rows of 32 {unit}", n_rows=2**35 + 1, row_len=32)
        add(name, OK, None, n_rows=0, row_len=0, rows=0, out=0)
        add(name, BAD_ARG, "null buffer", row_len=0, rows=0, out=0)   # no row data: rows is not looked at, out is
        if strided:
            add(name, BAD_ARG, "row stride 3 below the row length 4", forms=[True], row_len=4, row_stride=3)
            add(name, ALLOC, f"{2**35 + 1} rows of 32 {unit}", forms=[True], n_rows=2**35 + 1, row_len=4, row_stride=32)
            add(name, BAD_ARG, None, forms=[True], row_len=LONG, row_stride=3)   # two faults: the stride is looked at first

    def tree(name, max_log2n, no_columns=NO_COLUMNS, strided=True):
        add(name, BAD_ARG, no_columns, **{"leaves" if name.startswith("pedersen") else "columns": 0})
        add(name, BAD_ARG, no_columns, forms=[False], root=0)
        add(name, BAD_ARG, no_columns, forms=[True], nodes=0)
        add(name, BAD_ARG, ALIGN, forms=[True], **{"leaves" if name.startswith("pedersen") else "columns": A + 8})
        add(name, BAD_ARG, ALIGN, forms=[True], nodes=B + 8)
        add(name, ALLOC, f"2^{max_log2n + 1} leaves", log2n=max_log2n + 1)
        add(name, BAD_ARG, None, forms=[True], nodes=B + 8, log2n=max_log2n + 1)   # two faults: the alignment is looked at first
        if strided:
            add(name, BAD_ARG, NO_COLUMNS, n_cols=0)
            add(name, BAD_ARG, "column stride 7 below the column length", forms=[True], n_cols=2, col_stride=7)
            add(name, ALLOC, None, forms=[True], col_stride=7, log2n=max_log2n + 1)   # two faults: the leaf count is looked at first

    flat("poseidon_permute", ["states", "out"], "Poseidon")
    flat("poseidon_hash", ["x", "y", "out"], "Poseidon")
    flat("poseidon_hash_single", ["x", "out"], "Poseidon")
    add("poseidon_hash_single", ALLOC, f"{2**40 + 1} rows of 1 elements", n=2**40 + 1)
    row_shape("poseidon_hash_many", "Poseidon", "elements", strided=False)
    tree("poseidon_commit_columns", 31)
    add("poseidon_commit_columns", BAD_ARG, "bad leaf mode 2", mode=2)
    add("poseidon_commit_columns", BAD_ARG, "LW_POSEIDON_LEAF_SINGLE (TreePoseidon) commits one column, not 2", mode=0, n_cols=2)
    add("poseidon_commit_columns", BAD_ARG, NO_COLUMNS, mode=0, n_cols=0)
    add("poseidon_commit_columns", BAD_ARG, None, mode=2, log2n=32)   # two faults

    for name in ("rpo_permute", "rpo_hash", "rpo_commit_columns"):
        key = "sel" if name == "rpo_commit_columns" else "level"
        for bad in (-1, 2):
            add(name, BAD_ARG, LEVEL(bad), **{key: bad})
    flat("rpo_permute", ["states", "out"], "RPO")
    add("rpo_permute", BAD_ARG, None, level=2, n=BIG)   # two faults
    row_shape("rpo_hash", "RPO", "words", strided=True)
    tree("rpo_commit_columns", 30)

    add("pedersen_table", BAD_ARG, "null buffer", out=0)
    flat("pedersen_hash", ["x", "y", "out"], "Pedersen")
    flat("pedersen_add_affine", ["p", "z", "q", "out"], "Pedersen")
    tree("pedersen_commit_leaves", 31, no_columns="null buffer", strided=False)
    for n_cols in (0, 2):
        add("pedersen_commit_leaves", BAD_ARG, f"a Pedersen tree commits one column of leaf values, not {n_cols}", n_cols=n_cols)
    add("pedersen_commit_leaves", BAD_ARG, None, n_cols=2, log2n=32)   # two faults

    for name in ("monolith_constants", "monolith_permute", "monolith_layer"):
        for w in (0, 4, 10, 28):
            add(name, BAD_ARG, WIDTH(w), width=w)
    for name in ("monolith_constants", "monolith_permute", "monolith_layer", "monolith_hash", "monolith_compress", "monolith_commit_columns"):
        for r in (0, 16):
            add(name, BAD_ARG, ROUNDS(r), rounds=r)
    add("monolith_constants", BAD_ARG, "null buffer", rc=0)
    add("monolith_constants", BAD_ARG, "null buffer", mds=0)
    flat("monolith_permute", ["states", "out"], "Monolith")
    add("monolith_layer", BAD_ARG, "bad Monolith layer 3", layer=3)
    flat("monolith_layer", ["states", "out"], "Monolith")
    row_shape("monolith_hash", "Monolith", "words", strided=True)
    flat("monolith_compress", ["left", "right", "out"], "Monolith")
    tree("monolith_commit_columns", 30)
    return out


def test_every_hash_entry_refuses_one_fault_at_a_time_with_its_status_and_text():
    L = _library()
    cases = _cases(L)
    hash_exports = {s for s in _lib.EXPORTS if s.startswith(("lw_poseidon_", "lw_rpo_", "lw_pedersen_", "lw_monolith_"))}
    assert {"lw_" + label.split()[0] for label, _, _, _ in cases} == hash_exports
    assert len({label for label, _, _, _ in cases}) == len(cases)
    got, expected = {}, {}
    for label, call, status, text in cases:
        assert L.lw_rpo_permute(i(99), None, sz(0), None) == BAD_ARG   # a text no case expects, so a stale one cannot pass
        rc = call()
        got[label] = (rc, L.lw_hip_last_error().decode() if text is not None else None)
        expected[label] = (status, text)
    assert got == expected
