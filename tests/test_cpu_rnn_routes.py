"""The dispatch policy of the recurrent kernels (csrc/rnn.h rnn_route, followed by launch_rnn_recurrent and by rnn_bptt.hip's
launch_rnn_bptt) asked through tn_dbg_rnn_route, which touches no device: the training shape tables of tests/tools/rnn_train_shapes.py
reach every instantiation for both cells, and the policy's edges lie where the kernels' launch bounds need them.  No GPU needed."""
import ctypes as C

import pytest

from tools import rnn_train_shapes as RS


@pytest.fixture(scope="module")
def lib():
    from tennis_amd import _lib
    return _lib.load()


def _reached_head(lib, cell, rows):
    return {RS.route_name(lib, c, B, H, 2) for c, B, T, F, H in rows if c == cell}


def _reached_gnmt(lib, cell, cases):
    return {RS.route_name(lib, cell, cfg["B"], cfg["H"], d) for cfg in cases if cfg["cell"] == cell for d in RS.gnmt_layer_dirs(cfg)}


@pytest.mark.parametrize("cell", ["gru", "lstm"])
def test_tables_reach_every_route(lib, cell):
    head = _reached_head(lib, cell, RS.head_cases())
    assert head == set(RS.ROUTES), (cell, sorted(set(RS.ROUTES) ^ head))          # the head table alone: all six, and no unnamed seventh
    both = head | _reached_gnmt(lib, cell, RS.gnmt_cases())
    assert both == set(RS.ROUTES), (cell, sorted(set(RS.ROUTES) ^ both))
    # with valid_len and final-state gradients: the two prefixes no captioner test reached before, and the 4-row kernel
    assert {"nb1_kr64", "nb1_kr96", "nb4"} <= _reached_gnmt(lib, cell, RS.gnmt_cases())


@pytest.mark.parametrize("cell", ["gru", "lstm"])
def test_a_route_losing_its_only_row_is_noticed(lib, cell):
    """what test_tables_reach_every_route rests on: without the rows of any one route the set reached is no longer the full one"""
    rows = RS.head_cases()
    for r in RS.ROUTES:
        kept = [row for row in rows if not (row[0] == cell and RS.route_name(lib, cell, row[1], row[4], 2) == r)]
        assert len(kept) < len(rows) and _reached_head(lib, cell, kept) == set(RS.ROUTES) - {r}


def test_every_row_is_a_legal_shape(lib):
    for cell, B, T, F, H in RS.head_cases():
        assert H % 4 == 0 and RS.GATES[cell] * H <= 1024 and min(B, T, F) > 0
    for cfg in RS.gnmt_cases():
        assert cfg["H"] % 4 == 0 and RS.GATES[cfg["cell"]] * cfg["H"] <= 1024 and 0 <= cfg["nbi"] <= cfg["nl"]
    assert len(set(RS.head_cases())) == len(RS.head_cases())


@pytest.mark.parametrize("cell", ["gru", "lstm"])
def test_rows_per_workgroup_edges(lib, cell):
    for dirs, last1, first4 in ((2, 508, 509), (1, 1020, 1021)):
        for H in (8, 100, 128):
            assert RS.route(lib, cell, last1, H, dirs)[0] == 1 and RS.route(lib, cell, first4, H, dirs)[0] == 4
    assert RS.route(lib, cell, 1, 32, 1)[0] == 1 and RS.route(lib, cell, 4096, 32, 1)[0] == 4
    # four rows per workgroup: never a register prefix, never the big form - whatever the width
    for H in (8, 64, 96, 128, 168, 192, 252, 256):
        assert RS.route(lib, cell, 509, H, 2) == (4, 0, 0)
        assert RS.route(lib, cell, 1021, H, 1) == (4, 0, 0)


@pytest.mark.parametrize("cell", ["gru", "lstm"])
def test_h256_is_big_only_at_one_row_per_workgroup(lib, cell):
    for B, dirs in ((1, 1), (3, 2), (508, 2), (1020, 1)):
        nb, _, big = RS.route(lib, cell, B, 256, dirs)
        assert (nb, big) == (1, 1)
    for B, dirs in ((509, 2), (516, 2), (1021, 1)):
        assert RS.route(lib, cell, B, 256, dirs) == (4, 0, 0)
    top = 340 if cell == "gru" else 252
    for H in range(4, top + 1, 4):                                  # no other width is big
        if H != 256:
            assert RS.route(lib, cell, 3, H, 2)[2] == 0, H


def test_prefix_edges(lib):
    """kr over every legal width at one row per workgroup: the prefix fits the registers that the block size leaves (a 128-value prefix
    under the 512-thread launch bound, 96 under 768, 64 under 1024) and never exceeds the column"""
    want = {"gru": [(4, 60, 0), (64, 92, 64), (96, 124, 96), (128, 168, 128), (172, 252, 96), (260, 340, 64)],
            "lstm": [(4, 60, 0), (64, 92, 64), (96, 124, 96), (128, 128, 128), (132, 192, 96), (196, 252, 64)]}
    for cell, spans in want.items():
        g = RS.GATES[cell]
        seen = set()
        for lo, hi, kr in spans:
            for H in range(lo, hi + 1, 4):
                for B, dirs in ((1, 1), (3, 2), (508, 2)):
                    assert RS.route(lib, cell, B, H, dirs) == (1, kr, 0), (cell, H, B, dirs)
                assert kr <= H and g * H <= {128: 512, 96: 768, 64: 1024, 0: 1024}[kr]
                seen.add(H)
        assert seen == set(range(4, 1024 // g + 1, 4)) - {256}
    # the edges by name
    for cell, edges in (("gru", [(60, 0), (64, 64), (92, 64), (96, 96), (124, 96), (128, 128), (168, 128), (172, 96)]),
                        ("lstm", [(60, 0), (64, 64), (92, 64), (96, 96), (124, 96), (128, 128), (132, 96), (192, 96), (196, 64)])):
        for H, kr in edges:
            assert RS.route(lib, cell, 3, H, 2)[1] == kr, (cell, H)


def test_hook_refuses_what_the_launchers_refuse(lib):
    nb, kr, big = C.c_int(), C.c_int(), C.c_int()
    out = (C.byref(nb), C.byref(kr), C.byref(big))
    assert lib.tn_dbg_rnn_route(3, 3, 64, 2, *out) == 0
    assert lib.tn_dbg_rnn_route(2, 3, 64, 2, *out) != 0             # gates
    assert lib.tn_dbg_rnn_route(3, 3, 66, 2, *out) != 0             # hidden % 4
    assert lib.tn_dbg_rnn_route(4, 3, 260, 2, *out) != 0            # 1040 threads
    assert lib.tn_dbg_rnn_route(3, 3, 344, 2, *out) != 0            # 1032 threads
    assert lib.tn_dbg_rnn_route(3, 0, 64, 2, *out) != 0
    assert lib.tn_dbg_rnn_route(3, 3, 64, 3, *out) != 0
    assert lib.tn_dbg_rnn_route(3, 3, 64, 2, None, C.byref(kr), C.byref(big)) != 0
