"""The training shapes that pin every instantiation of the recurrent kernels (csrc/rnn.hip with `save`, csrc/rnn_bptt.hip's BPTT kernels)
against float64, and the names of the routes they are chosen to reach.  Shared by tests/test_cpu_rnn_routes.py (the tables reach
every route, asked of the library's own dispatch policy through tn_dbg_rnn_route: no GPU) and tests/test_gpu_rnn_train_routes.py
(the steps themselves).

A route is one template instantiation per cell type, picked by csrc/rnn.h rnn_route from (gates, B, H, dirs):

  nb1_kr0    H < 64                                            no register-resident prefix of the W_hh column
  nb1_kr64   GRU H 64..92 (and 260..340); LSTM 64..92, 196..252  64-value prefix, 1024-thread bound
  nb1_kr96   GRU H 96..124, 172..252; LSTM 96..124, 132..192   96-value prefix, 768-thread bound
  nb1_kr128  GRU H 128..168; LSTM H = 128                      128-value prefix, 512-thread bound
  nb1_big    H = 256 at one row per workgroup                  registers + LDS + stream
  nb4        ((B + 3) / 4) * dirs >= 256                       four rows per workgroup, no prefix

A new instantiation needs a new name in ROUTES and a row here that reaches it: the CPU test compares the routes reached with ROUTES.
"""
import ctypes as C

GATES = {"gru": 3, "lstm": 4}
ROUTES = ("nb1_kr0", "nb1_kr64", "nb1_kr96", "nb1_kr128", "nb1_big", "nb4")

# Temporal head (bidirectional, no valid_len, no final-state gradient): (cell or None for both, B, T, F, H, what the row is there for)
HEAD_SHAPES = [
    (None, 4, 6, 16, 64, "prefix 64 alone"),
    (None, 3, 5, 16, 68, "prefix 64 + 4-wide tail"),
    (None, 3, 5, 16, 92, "prefix 64 + one streamed group + tail"),
    ("lstm", 3, 4, 16, 196, "prefix 64 on a near-full block"),
    ("lstm", 3, 4, 16, 252, "prefix 64, 1008 threads"),
    ("gru", 3, 4, 16, 340, "prefix 64, 1020 threads: the GRU widths past 256"),
    (None, 4, 6, 16, 96, "prefix 96 alone"),
    (None, 3, 5, 16, 100, "prefix 96 + tail"),
    ("gru", 3, 5, 16, 172, "prefix 96 + streamed groups + tail"),
    ("gru", 3, 4, 16, 252, "prefix 96, 756 threads"),
    ("lstm", 3, 5, 16, 132, "prefix 96 + two streamed groups + tail"),
    ("lstm", 3, 5, 16, 192, "prefix 96, exactly 768 threads"),
    ("gru", 3, 5, 16, 168, "prefix 128 + 2 x 16 + 8"),
    (None, 3, 5, 16, 128, "prefix 128 alone (LSTM: its only width)"),
    (None, 3, 4, 16, 256, "registers + LDS + stream"),
    (None, 3, 5, 16, 36, "no prefix, ragged"),
    (None, 3, 5, 16, 60, "no prefix, ragged, last width below the prefix"),
    (None, 520, 3, 8, 32, "four rows per workgroup"),
    (None, 517, 2, 8, 36, "four rows: the last workgroup holds one real row and three padded ones"),
    (None, 509, 2, 8, 100, "four rows at the threshold, a prefix-eligible width on the prefix-less kernel"),
    (None, 516, 2, 8, 256, "four rows: H = 256 off the big route"),
]

# Captioner step (valid_len and final-state gradients): both cells unless `cell` is set; encoder layers below num_bi_layers are
# bidirectional, the others unidirectional
_SMALL = dict(B=3, F=16, E=12, V=20, L=5, nl=2, nbi=1)
GNMT_CASES = [
    dict(_SMALL, seed=21, T=7, H=64),
    dict(_SMALL, seed=22, T=7, H=100),
    dict(_SMALL, seed=23, T=6, H=192),
    dict(_SMALL, seed=24, T=6, H=196, cell="lstm"),
    dict(seed=25, B=517, T=4, F=8, H=8, E=6, V=12, L=4, nl=2, nbi=1),      # bidirectional layer on the 4-row kernel, padded rows
    dict(seed=26, B=1030, T=3, F=8, H=8, E=6, V=12, L=4, nl=2, nbi=0),     # unidirectional layers on the 4-row kernel
]


def cells_of(cell):
    return ("gru", "lstm") if cell is None else (cell,)


def head_cases():
    """-> [(cell, B, T, F, H)], every row for every cell it names"""
    return [(c, B, T, F, H) for cell, B, T, F, H, _ in HEAD_SHAPES for c in cells_of(cell)]


def gnmt_cases():
    """-> [dict for test_gpu_gnmt_train._case and GNMTTrainer], every case for every cell it names"""
    return [dict(cfg, cell=c) for cfg in GNMT_CASES for c in cells_of(cfg.get("cell"))]


def gnmt_layer_dirs(cfg):
    """directions of the encoder's layers, bottom up"""
    return [2 if i < cfg["nbi"] else 1 for i in range(cfg["nl"])]


def route(lib, cell, B, H, dirs):
    """(nb, kr, big) of the library's dispatch policy (tn_dbg_rnn_route; no device is touched)"""
    nb, kr, big = C.c_int(-1), C.c_int(-1), C.c_int(-1)
    rc = lib.tn_dbg_rnn_route(GATES[cell], B, H, dirs, C.byref(nb), C.byref(kr), C.byref(big))
    if rc != 0:
        raise RuntimeError(f"tn_dbg_rnn_route({cell}, B={B}, H={H}, dirs={dirs}) failed ({rc})")
    return nb.value, kr.value, big.value


def route_name(lib, cell, B, H, dirs):
    nb, kr, big = route(lib, cell, B, H, dirs)
    if big:
        return "nb1_big"
    return "nb4" if nb == 4 else f"nb1_kr{kr}"
