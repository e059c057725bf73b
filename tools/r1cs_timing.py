#!/usr/bin/env python3
"""The resident R1CS on the device (csrc/r1cs.hip): the two sparse products next to the bytes they move, on a skewed and
on an evenly loaded system, and Groth16's h from a witness next to the h pipeline alone.
  FIELD:LOG  for one field and 2^LOG rows and columns, in one process: r1cs.matvec_device (all three products) and
             r1cs.bind_rows_device on tools/inputs.r1cs_system, skewed (the row and column profile of the circom Poseidon
             circuit) and uniform (the same number of entries spread evenly), alternating with a device-to-device copy of
             2^LOG elements.  Each figure is set against its bytes at the copy's rate: the index arrays read once (row
             offsets and entries, 4 bytes each), a 32-byte value per general entry, a 32-byte gathered element per entry,
             and the outputs written (three for matvec, one for bind_rows).
  h:LOG      groth16.h_from_witness_device of a 2^LOG-row uniform Fr381 system at num_gates = 2^LOG next to
             groth16.calculate_h_coefficients_device alone at the same num_gates.
A sample is CALLS calls enqueued back to back and one synchronise; the figure is the sample's time per call.
Every step is a process of its own under `timeout -k 10`, chained with &&: a step that fails or hangs ends the run.
usage: r1cs_timing.py [--out FILE]        (r1cs_timing.py --step NAME runs one step)"""
import argparse
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STEPS = [("stark252:20", 240), ("fr381:20", 240), ("stark252:22", 420), ("fr381:22", 420), ("h:20", 300)]
REPS = 5
CALLS = 20


def sample(fn):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(CALLS):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / CALLS


def rounds(fns):
    """{name: [REPS samples]} of the callables, alternating, after one warm-up sample of each"""
    for fn in fns.values():
        sample(fn)
    out = {k: [] for k in fns}
    for _ in range(REPS):
        for k, fn in fns.items():
            out[k].append(sample(fn))
    return out


def fmt(v):
    return f"{statistics.median(v):8.3f} ms [{min(v):8.3f} .. {max(v):8.3f}]"


def system_bytes(mats, n_lists_in, n_out, outputs, one, minus_one):
    """bytes a product over these matrices has to move: offsets and entries once, a value per general entry, a gathered
    element per entry, the outputs"""
    import numpy as np
    total = outputs * n_out * 32
    for rp, ci, va in mats:
        general = int(np.count_nonzero((va != one).any(axis=1) & (va != minus_one).any(axis=1)))
        total += (n_lists_in + 1) * 4 + ci.shape[0] * (4 + 32) + general * 32
    return total


def step(name):
    import numpy as np
    import torch
    from lambda_elliptic_curves_amd import groth16, multilinear, r1cs
    from tools import inputs
    field, log = name.split(":")
    n = 1 << int(log)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).cuda()
    if field == "h":
        F = inputs.field_pairs()["fr381"][0]
        sys_ = r1cs.R1cs(F, n, n, inputs.r1cs_system("fr381", n, n, False, 7))
        t_w = dev(inputs.rand_elems("fr381", n, 8))
        t_lro = [dev(inputs.rand_elems("fr381", n, 9 + k)) for k in range(3)]
        t_out = torch.empty((2 * n, 4), dtype=torch.int64, device="cuda")
        got = rounds({"witness": lambda: groth16.h_from_witness_device(sys_, t_w, n, t_out),
                      "h alone": lambda: groth16.calculate_h_coefficients_device(*t_lro, n, n, t_out)})
        print(f"RESULT groth16 h at 2^{log} gates (fr381): from the witness {fmt(got['witness'])}, lw_groth16_h_coefficients_device alone "
              f"{fmt(got['h alone'])}, ratio {statistics.median(got['witness']) / statistics.median(got['h alone']):.3f}")
        return 0
    F = inputs.field_pairs()[field][0]
    p = multilinear.MODULI[F.field]
    word = lambda v: np.array([(v >> (64 * (3 - k))) & ((1 << 64) - 1) for k in range(4)], dtype=np.uint64)
    one, minus_one = word((1 << 256) % p), word(p - (1 << 256) % p)
    t_z, t_e = dev(inputs.rand_elems(field, n, 1)), dev(inputs.rand_elems(field, n, 2))
    c3 = inputs.rand_elems(field, 3, 3)
    outs = [torch.empty((n, 4), dtype=torch.int64, device="cuda") for _ in range(3)]
    dst = torch.empty_like(t_z)
    fns, nbytes = {"copy": lambda: dst.copy_(t_z)}, {}
    keep = []
    for tag, skewed in (("skewed", True), ("uniform", False)):
        mats = inputs.r1cs_system(field, n, n, skewed, 4)
        h = r1cs.R1cs(F, n, n, mats)
        keep.append(h)
        nbytes["matvec " + tag] = system_bytes(mats, n, n, 3, one, minus_one)
        nbytes["bind " + tag] = system_bytes(mats, n, n, 1, one, minus_one)
        fns["matvec " + tag] = lambda h=h: h.matvec_device(t_z, n, outs)
        fns["bind " + tag] = lambda h=h: h.bind_rows_device(t_e, c3, n, outs[0])
        longest = max(int(np.diff(rp.astype(np.int64)).max()) for rp, _, _ in mats)
        heavy = max(int(np.bincount(ci, minlength=1).max()) for _, ci, _ in mats)
        print(f"RESULT {field} 2^{log} {tag}: {sum(ci.shape[0] for _, ci, _ in mats)} entries, longest row {longest}, heaviest column {heavy}")
    got = rounds(fns)
    cp = statistics.median(got["copy"])
    rate = 2 * n * 32 / cp / 1e6
    print(f"RESULT {field} 2^{log} copy of {n * 32 >> 20} MiB: {fmt(got['copy'])} = {rate:.0f} GB/s read + write")
    for k in fns:
        if k == "copy":
            continue
        med = statistics.median(got[k])
        floor = nbytes[k] / rate / 1e6
        print(f"RESULT {field} 2^{log} {k:15s}: {fmt(got[k])}; {nbytes[k] / 1e6:8.1f} MB at the copy's rate -> {floor:.3f} ms = {floor / med:.3f} of the call")
    for op in ("matvec", "bind"):
        print(f"RESULT {field} 2^{log} {op}: skewed / uniform = {statistics.median(got[op + ' skewed']) / statistics.median(got[op + ' uniform']):.3f}")
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r1cs.txt"))
    ap.add_argument("--step")
    args = ap.parse_args()
    if args.step:
        return step(args.step)
    me = os.path.abspath(__file__)
    chain = " && ".join(f"timeout -k 10 {limit} {sys.executable} {me} --step {name}" for name, limit in STEPS)
    run = subprocess.run(chain, shell=True, capture_output=True, text=True, cwd=ROOT)
    lines = [f"# resident R1CS: wall ms per call, median [min .. max] of {REPS} samples of {CALLS} calls each after a warm-up sample, the "
             "forms alternating, stream synchronised per sample"]
    lines += [ln[7:] for ln in run.stdout.splitlines() if ln.startswith("RESULT")]
    if run.returncode:
        lines.append(f"# the chain stopped with exit status {run.returncode}: {(run.stdout[-400:] + run.stderr[-400:]).strip()}")
    print("\n".join(lines), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return run.returncode


if __name__ == "__main__":
    sys.exit(main())
