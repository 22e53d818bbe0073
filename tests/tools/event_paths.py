"""What the GPU tests of the two path decoders share (tests/test_gpu_event_viterbi.py, tests/test_gpu_event_transitions.py): layouts
and row modes placed from the chain kernels' tile G, the check of a call's events against its own frames, and a spy on the library."""
import numpy as np

from tools import events_ref as ER


def _geometry():
    from tennis_amd.engine import event_decoder_switch_geometry
    return event_decoder_switch_geometry()


G = _geometry()


def to_numpy(d):
    return {k: v.cpu().numpy() for k, v in d.items()}


def layout(m, kind):
    """video-start flags: 0 lengths 1, 2 and then exactly G; 1 lengths 1, 2, G - 3 and the rest (G + 3 at m = 2 G + 3: two tiles);
    2 one video over everything (three tiles at m = 2 G + 3)"""
    start = np.zeros(m, np.int32)
    for at in {0: (1, 3, 3 + G), 1: (1, 3, G), 2: ()}[kind]:
        if at < m:
            start[at] = 1
    return start


def rows_of(rng, m, mode):
    """the identity, a permutation of a larger N, or that with entries outside [0, N) -> (N, rows)"""
    n = m if mode == 0 else m + 37
    rows = np.arange(m) if mode == 0 else rng.permutation(n)[:m]
    if mode == 2:
        rows = rows.copy()
        rows[::5] = rng.choice([-3, -1, n, n + 9, 2 ** 31 - 1, -2 ** 31], len(rows[::5]))
    return n, rows.astype(np.int64)


def check_events_of_own_frames(got, start):
    from tennis_amd.events import label_runs
    first, last, cls = label_runs(got["label"], start)
    assert np.array_equal(got["first"], first) and np.array_equal(got["last"], last) and np.array_equal(got["cls"], cls)
    assert got["first"].dtype == np.int32 and got["score"].dtype == np.float32
    conf64 = got["conf"].astype(np.float64)
    for a, b, sc, pk in zip(first, last, got["score"], got["peak"]):
        assert pk == got["conf"][a:b + 1].max()
        assert abs(float(sc) - conf64[a:b + 1].mean()) <= ER.mean_bound(b - a + 1)


class Spy:
    """the library with every call recorded"""

    def __init__(self, lib, calls):
        self._lib, self._calls = lib, calls

    def __getattr__(self, name):
        self._calls.append(name)
        return getattr(self._lib, name)
