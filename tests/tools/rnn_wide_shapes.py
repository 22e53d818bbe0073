"""The shapes that pin the wide recurrent kernels (csrc/rnn.hip rnn_recurrent_wide_kernel, csrc/rnn_bptt.hip rnn_bptt_wide_kernel:
1024 < gates*H <= 2048, two gate rows per thread) against float64, and the names of the code paths they are chosen to reach.  Shared by
tests/test_cpu_rnn_wide_routes.py (the table reaches every path, asked of the library's own policy through tn_dbg_rnn_wide_route: no
GPU) and tests/test_gpu_rnn_wide.py (the kernels themselves).

A path is what a shape makes of one instantiation <cell, nb>, from csrc/rnn.h rnn_wide_route and the kernels' loops:

  nb1 | nb4        batch rows per workgroup; 4 from ((B + 3) / 4) * dirs >= 256, the threshold of rnn_route
  full | ragged    threads * 2 == gates*H (every thread owns a second row) or > gates*H (the guard on row j + threads works)
  tail | notail    H % 16 != 0: the 4-wide loop runs behind the 16-wide streamed one

The block is half the gate rows in whole waves, so `full` needs gates*H % 128 == 0, which makes H a multiple of 32: full_tail does not
exist, and the CPU test proves that from the policy.  The smallest shapes that reach every edge: T 2..6, F 8..16.
"""
import ctypes as C

GATES = {"gru": 3, "lstm": 4}
ROUTES = ("nb1_ragged_tail", "nb1_ragged_notail", "nb1_full_notail", "nb4_ragged_tail", "nb4_ragged_notail", "nb4_full_notail")

# (cell or None for both, B, T, F, H, dirs, what the row is there for)
SHAPES = [
    ("gru", 3, 6, 16, 344, 2, "1032 rows, the first width past the old limit: 576 threads, 456 own a second row"),
    ("lstm", 3, 6, 16, 260, 2, "1040 rows, the first width past the old limit"),
    ("gru", 3, 4, 12, 500, 2, "4-wide tail of 4 behind 31 streamed groups, 1500 rows on 768 threads"),
    ("lstm", 3, 4, 12, 380, 2, "4-wide tail of 12, 1520 rows on 768 threads"),
    (None, 3, 4, 12, 400, 2, "no tail, ragged second row"),
    ("gru", 3, 4, 8, 384, 2, "1152 rows on 576 threads: every thread owns two rows"),
    ("gru", 3, 3, 8, 680, 2, "2040 rows on 1024 threads: the widest GRU"),
    ("lstm", 3, 3, 8, 512, 2, "2048 rows on 1024 threads, exactly full: the widest LSTM"),
    ("gru", 3, 5, 16, 344, 1, "unidirectional"),
    ("gru", 517, 2, 8, 344, 2, "four rows per workgroup: the last one holds one real row and three padded ones"),
    ("lstm", 517, 2, 8, 260, 2, "four rows per workgroup: the last one holds one real row and three padded ones"),
    ("gru", 517, 2, 8, 352, 2, "four rows, no tail, ragged second row"),
    ("lstm", 517, 2, 8, 272, 2, "four rows, no tail, ragged second row"),
    ("gru", 517, 2, 8, 384, 2, "four rows, every thread owns two gate rows"),
    ("lstm", 517, 2, 8, 288, 2, "four rows, every thread owns two gate rows"),
]

# The temporal head takes the max over T, whose gradient goes to the step that holds the maximum: where two steps of a (row, unit) lie
# within rounding of each other, float32 and float64 may pick different steps, and one such flip moves a gradient by about 3e-3 of its
# maximum - an error of the comparison, not of a kernel.  Among the 517 x 2H x 2 values of the large-batch rows the closest pair
# is typically 1e-7 apart, so those rows carry a seed (of test_gpu_train._setup) at which the float32 oracle's closest pair is at least
# HEAD_MIN_GAP apart - eight units in the last place of an h in [0.5, 1), h lies in (-1, 1) - found on the oracle alone; the GPU
# test asserts the gap before it compares.  Seed 4, the seed of test_gpu_rnn_train_routes.py, everywhere else.
HEAD_MIN_GAP = 5e-7
HEAD_SEEDS = {("lstm", 517, 260): 17, ("gru", 517, 352): 23, ("lstm", 517, 272): 6, ("gru", 517, 384): 15}

# Captioner step (valid_len, final-state gradients; layer 0 bidirectional, the others unidirectional)
_SMALL = dict(B=3, F=16, E=12, V=20, L=5, nl=2, nbi=1)
GNMT_CASES = [
    dict(_SMALL, seed=31, cell="gru", T=6, H=344),
    dict(_SMALL, seed=32, cell="lstm", T=6, H=260),
    dict(_SMALL, seed=33, cell="lstm", nl=3, T=5, H=512),
]

# Inference: encode + beam search
_BEAM = dict(proj_scale=30.0, F=32, E=12, V=30)
BEAM_CASES = [
    dict(_BEAM, seed=41, cell="gru", H=344, B=3, T=9, beam=4, max_length=10),
    dict(_BEAM, seed=42, cell="lstm", H=260, B=3, T=9, beam=4, max_length=10),
    dict(_BEAM, seed=43, cell="lstm", H=512, nl=3, nbi=2, B=2, T=7, beam=3, max_length=8),
    dict(_BEAM, seed=44, cell="gru", H=680, B=2, T=7, beam=3, max_length=8),
]

# Bit identity of the wide kernels with the default routes under tn_dbg_rnn_force_wide: (cell, B, T, F, H)
FORCED_CASES = [(c, B, 4 if B == 3 else 2, 8, H) for c in ("gru", "lstm") for H in (64, 100, 256) for B in (3, 517)]


def cells_of(cell):
    return ("gru", "lstm") if cell is None else (cell,)


def cases():
    """-> [(cell, B, T, F, H, dirs)], every row for every cell it names"""
    return [(c, B, T, F, H, d) for cell, B, T, F, H, d, _ in SHAPES for c in cells_of(cell)]


def head_cases():
    """the rows a temporal head (always bidirectional) can run -> [(cell, B, T, F, H)]"""
    return [(c, B, T, F, H) for c, B, T, F, H, d in cases() if d == 2]


def head_seed(cell, B, H):
    return HEAD_SEEDS.get((cell, B, H), 4)


def wide_route(lib, cell, B, H, dirs):
    """(threads, rows, nb, lds_fwd, lds_bwd) of the library's policy (tn_dbg_rnn_wide_route; no device is touched)"""
    th, rows, nb = C.c_int(-1), C.c_int(-1), C.c_int(-1)
    lf, lb = C.c_int64(-1), C.c_int64(-1)
    rc = lib.tn_dbg_rnn_wide_route(GATES[cell], B, H, dirs, C.byref(th), C.byref(rows), C.byref(nb), C.byref(lf), C.byref(lb))
    if rc != 0:
        raise RuntimeError(f"tn_dbg_rnn_wide_route({cell}, B={B}, H={H}, dirs={dirs}) failed ({rc})")
    return th.value, rows.value, nb.value, lf.value, lb.value


def route_name(lib, cell, B, H, dirs):
    th, rows, nb, _, _ = wide_route(lib, cell, B, H, dirs)
    full = th * rows == GATES[cell] * H
    return f"nb{nb}_{'full' if full else 'ragged'}_{'tail' if H % 16 else 'notail'}"
