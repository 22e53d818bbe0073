"""The dispatch policy of the wide recurrent kernels (csrc/rnn.h rnn_wide_route, followed by launch_rnn_recurrent and by rnn_bptt.hip's
launch_rnn_bptt for 1024 < gates*H <= 2048) asked through tn_dbg_rnn_wide_route, which touches no device: what the hook refuses, the launch
bounds every legal shape keeps, the rows-per-workgroup edges, and that the shape table of tests/tools/rnn_wide_shapes.py reaches every
code path of the kernels for both cells.  No GPU needed."""
import ctypes as C

import pytest

from tools import rnn_wide_shapes as WS

LDS_MAX = 160 * 1024


@pytest.fixture(scope="module")
def lib():
    from tennis_amd import _lib
    return _lib.load()


def _widths(cell):
    g = WS.GATES[cell]
    return range(1024 // g // 4 * 4 + 4, 2048 // g + 1, 4)       # gru 344 .. 680, lstm 260 .. 512


def test_hook_refuses_what_the_wide_kernels_do_not_serve(lib):
    th, rows, nb, lf, lb = C.c_int(), C.c_int(), C.c_int(), C.c_int64(), C.c_int64()
    out = (C.byref(th), C.byref(rows), C.byref(nb), C.byref(lf), C.byref(lb))
    assert lib.tn_dbg_rnn_wide_route(3, 3, 344, 2, *out) == 0
    assert lib.tn_dbg_rnn_wide_route(4, 3, 512, 2, *out) == 0
    assert lib.tn_dbg_rnn_wide_route(3, 3, 340, 2, *out) != 0           # 1020 rows: the one-row-per-thread kernels
    assert lib.tn_dbg_rnn_wide_route(4, 3, 256, 2, *out) != 0           # 1024 rows
    assert lib.tn_dbg_rnn_wide_route(3, 3, 64, 2, *out) != 0
    assert lib.tn_dbg_rnn_wide_route(3, 3, 684, 2, *out) != 0           # 2052 rows
    assert lib.tn_dbg_rnn_wide_route(4, 3, 516, 2, *out) != 0           # 2064 rows
    assert lib.tn_dbg_rnn_wide_route(3, 3, 1000, 2, *out) != 0
    assert lib.tn_dbg_rnn_wide_route(3, 3, 346, 2, *out) != 0           # hidden % 4
    assert lib.tn_dbg_rnn_wide_route(2, 3, 400, 2, *out) != 0           # gates
    assert lib.tn_dbg_rnn_wide_route(5, 3, 400, 2, *out) != 0
    assert lib.tn_dbg_rnn_wide_route(3, 0, 400, 2, *out) != 0
    assert lib.tn_dbg_rnn_wide_route(3, 3, 400, 0, *out) != 0
    assert lib.tn_dbg_rnn_wide_route(3, 3, 400, 3, *out) != 0
    for i in range(5):                                                  # every output is needed
        args = list(out)
        args[i] = None
        assert lib.tn_dbg_rnn_wide_route(3, 3, 400, 2, *args) != 0
    # the narrow hook still answers for the narrow shapes only
    a, b, c = C.c_int(), C.c_int(), C.c_int()
    assert lib.tn_dbg_rnn_route(3, 3, 340, 2, C.byref(a), C.byref(b), C.byref(c)) == 0
    assert lib.tn_dbg_rnn_route(3, 3, 344, 2, C.byref(a), C.byref(b), C.byref(c)) != 0


@pytest.mark.parametrize("cell", ["gru", "lstm"])
def test_every_legal_shape_keeps_the_launch_bounds(lib, cell):
    g = WS.GATES[cell]
    seen = set()
    for H in _widths(cell):
        for B, dirs in ((1, 1), (3, 2), (508, 2), (509, 2), (517, 2), (1020, 1), (1021, 1), (4096, 2)):
            th, rows, nb, lf, lb = WS.wide_route(lib, cell, B, H, dirs)
            assert th <= 1024 and th % 64 == 0 and rows == 2 and th * rows >= g * H, (cell, H, B, dirs, th)
            assert th * rows - g * H < 128, (cell, H, th)                # half the rows in whole waves: no idle wave
            assert nb in (1, 4)
            assert lf == 4 * nb * H * (2 + g), (cell, H, nb, lf)         # h | gates | c
            assert lb == 4 * nb * H * ((2 if g == 4 else 1) + 2 * g), (cell, H, nb, lb)
            assert 0 < lf <= LDS_MAX and 0 < lb <= LDS_MAX
        seen.add(H)
    assert min(seen) * g > 1024 >= (min(seen) - 4) * g and max(seen) * g <= 2048 < (max(seen) + 4) * g
    assert WS.wide_route(lib, "lstm", 4096, 512, 2)[3:] == (48 * 1024, 80 * 1024)


@pytest.mark.parametrize("cell", ["gru", "lstm"])
def test_rows_per_workgroup_edges(lib, cell):
    """rnn_route's threshold: four rows from ((B + 3) / 4) * dirs >= 256, whatever the width"""
    for dirs, last1, first4 in ((2, 508, 509), (1, 1020, 1021)):
        for H in (_widths(cell)[0], 400, _widths(cell)[-1]):
            assert WS.wide_route(lib, cell, last1, H, dirs)[2] == 1 and WS.wide_route(lib, cell, first4, H, dirs)[2] == 4
    assert WS.wide_route(lib, cell, 1, 400, 1)[2] == 1 and WS.wide_route(lib, cell, 4096, 400, 1)[2] == 4


@pytest.mark.parametrize("cell", ["gru", "lstm"])
def test_table_reaches_every_path(lib, cell):
    # what exists at all, from the policy itself: every legal width at both rows-per-workgroup values (no full_tail: see the table's docstring)
    exists = {WS.route_name(lib, cell, B, H, 2) for H in _widths(cell) for B in (3, 517)}
    assert exists == set(WS.ROUTES), sorted(exists ^ set(WS.ROUTES))
    reached = {WS.route_name(lib, c, B, H, d) for c, B, T, F, H, d in WS.cases() if c == cell}
    assert reached == set(WS.ROUTES), (cell, sorted(set(WS.ROUTES) ^ reached))
    # ... and the temporal-head rows alone (the BPTT kernels)
    head = {WS.route_name(lib, c, B, H, 2) for c, B, T, F, H in WS.head_cases() if c == cell}
    assert head == set(WS.ROUTES), (cell, sorted(set(WS.ROUTES) ^ head))


@pytest.mark.parametrize("cell", ["gru", "lstm"])
def test_a_path_losing_its_only_row_is_noticed(lib, cell):
    """what test_table_reaches_every_path rests on: without the rows of any one path the set reached is no longer the full one"""
    rows = WS.cases()
    for r in WS.ROUTES:
        kept = [row for row in rows if not (row[0] == cell and WS.route_name(lib, cell, row[1], row[4], row[5]) == r)]
        left = {WS.route_name(lib, c, B, H, d) for c, B, T, F, H, d in kept if c == cell}
        assert len(kept) < len(rows) and left == set(WS.ROUTES) - {r}


def test_every_row_is_a_legal_wide_shape(lib):
    for cell, B, T, F, H, d in WS.cases():
        assert H % 4 == 0 and 1024 < WS.GATES[cell] * H <= 2048 and 2 <= T <= 6 and 8 <= F <= 16 and B > 0 and d in (1, 2)
    assert len(set(WS.cases())) == len(WS.cases())
    assert any(d == 1 for *_, d in WS.cases())
    # the edges by name: first widths past the old limit, the widest ones, a last workgroup of one real row
    have = {(c, H) for c, B, T, F, H, d in WS.cases()}
    assert {("gru", 344), ("lstm", 260), ("gru", 500), ("lstm", 380), ("gru", 680), ("lstm", 512)} <= have
    assert {(c, B) for c, B, T, F, H, d in WS.cases() if B > 3} == {("gru", 517), ("lstm", 517)} and 517 % 4 == 1
    for cfg in WS.GNMT_CASES + WS.BEAM_CASES:
        assert cfg["H"] % 4 == 0 and 1024 < WS.GATES[cfg["cell"]] * cfg["H"] <= 2048
    # the forced cases are narrow shapes on both sides of the rows-per-workgroup threshold
    for cell, B, T, F, H in WS.FORCED_CASES:
        assert WS.GATES[cell] * H <= 1024 and H % 4 == 0
    assert {B for _, B, *_ in WS.FORCED_CASES} == {3, 517} and {H for *_, H in WS.FORCED_CASES} == {64, 100, 256}
