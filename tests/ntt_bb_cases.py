"""The transform sizes of tests/test_gpu_ntt_babybear_edges.py, kept free of torch and of the library so that
tests/test_ntt_bb_shapes_cpu.py can check without a device which kernel instantiations they reach.

One entry per transform: (lgV, L, skip).  lgV = 0 is the base field (run in both word types, u32 and u64), lgV = 2 the
quartic extension (four u64 components per index).  2^L elements come out; skip = 0 is a plain transform (forward,
inverse, on a coset, out of place and in place), skip > 0 a low-degree extension of 2^(L - skip) coefficients with
blow-up 2^skip, whose first `skip` stages are not run.  No buffer holds more than 2^20 words (2^(L + lgV)).

The comment beside each entry is the plan as (stages of each pass, RXn = the kernel with an n-stage tile compiled in,
rt = the kernel that takes its tile shape from the parameters); test_ntt_bb_shapes_cpu.py derives the same from
csrc/ntt_plan.h and fails when an entry that alone reaches an instantiation is taken out."""

MAX_LOG_WORDS = 20

SIZES = (
    (0, 8, 0),    # [8 rt], a single pass
    (0, 12, 0),   # [6 rt][6 rt], the largest size without a compiled shape
    (0, 13, 0),   # [7 RX7][6 RX6]
    (0, 15, 0),   # [8 RX8][7 RX7]
    (0, 16, 0),   # [8 RX8][8 RX8]
    (0, 17, 0),   # [6 RX6][6 rt][5 rt]
    (0, 18, 0),   # [6 RX6][6 rt][6 RX6]
    (0, 20, 0),   # [7 RX7][7 RX7][6 RX6], the first compiled middle pass of the base field
    (0, 16, 1),   # [8 RX8][7 RX7], blow-up 2
    (0, 15, 3),   # [6 rt][6 RX6], blow-up 8
    (0, 18, 2),   # [8 RX8][8 RX8], blow-up 4
    (0, 13, 5),   # [8 RX8], a single compiled pass: only a low-degree extension has so few stages over a full tile; blow-up 32
    (0, 13, 6),   # [7 RX7], blow-up 64
    (0, 13, 7),   # [6 RX6], blow-up 128
    (2, 5, 0),    # [5 rt], a single pass
    (2, 9, 0),    # [5 rt][4 rt]
    (2, 11, 0),   # [6 RX6][5 rt]
    (2, 13, 0),   # [7 RX7][6 RX6]
    (2, 15, 0),   # [8 RX8][7 RX7]
    (2, 16, 0),   # [8 RX8][8 RX8]
    (2, 17, 0),   # [6 RX6][6 RX6][5 rt], the first compiled middle pass of the extension
    (2, 18, 0),   # [6 RX6][6 RX6][6 RX6]
    (2, 13, 2),   # [6 RX6][5 rt], blow-up 4
    (2, 11, 3),   # [8 RX8], a single compiled pass, blow-up 8
    (2, 11, 4),   # [7 RX7], blow-up 16
    (2, 11, 5),   # [6 RX6], blow-up 32
)

# sizes from which only `all-p-1` and `random` (the extension: two of the four rotations) run in every form
REDUCED_FROM_LOG_WORDS = 18


def sizes(lgV, lde):
    """(L, skip) of the entries of one word shape: the plain transforms or the low-degree extensions"""
    return [(L, skip) for v, L, skip in SIZES if v == lgV and (skip > 0) == lde]
