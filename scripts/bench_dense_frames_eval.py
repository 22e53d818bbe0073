"""Dense evaluation through a row table: (a) the table form of the windowed head against its arithmetic form on the same windows,
device time; (b) `evaluate` on a synthetic split of frames, loader route against --dense_windows, wall time.

(a) The shape of scripts/bench_window_head.py: one sequence of --rows rows, one window per row, F = 1024, H = 128, GRU and LSTM;
    ``WindowHead.forward`` (centre, lo, hi) against ``WindowHead.forward_rows`` on the table that spells the same windows out (the
    logits must be bit-equal; the table is built once, outside the timing, as ``TennisSet.window_table`` builds it once per split).
(b) ``evaluate.main`` in this process on a synthetic root (frames generated on the host from (video, frame), 224 x 224), window 8
    and 30: the whole call, and the evaluation loop's own "Time Taken" that the driver prints.

The routes alternate, --runs runs each; medians and spread (max - min) are recorded next to the runs (docs/measurement.md).
One JSON document -> profiles/dense_frames_eval_bench.json.

    python scripts/bench_dense_frames_eval.py [--rows 172047] [--window 30] [--frames_per_video 64] [--out profiles/dense_frames_eval_bench.json]
"""
import argparse
import contextlib
import io
import json
import os
import re
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), out


def stats(v):
    return dict(runs=[round(x, 3) for x in v], median=round(float(np.median(v)), 3), spread=round(float(max(v) - min(v)), 3))


def head_forms(a):
    from tennis_amd import weights as W
    from tennis_amd.engine import WindowHead
    n, T, feat, hidden, classes = a.rows, a.window, 1024, 128, 11
    dev = torch.device("cuda")
    centre = torch.arange(n, dtype=torch.int32, device=dev)
    lo, hi = torch.zeros_like(centre), torch.full_like(centre, n - 1)
    offs = (torch.arange(T, device=dev) - T // 2) * a.stride
    table = (centre[:, None].long() + offs[None, :]).clamp_(0, n - 1).to(torch.int32).contiguous()
    g = torch.Generator(device=dev)
    g.manual_seed(feat)
    feats = torch.randn((n, feat), generator=g, device=dev).abs_() * 0.5
    out = []
    for mode in ("gru", "lstm"):
        pre = f"bench_{mode}_"
        p = W.make_rnn_weights(3, mode, feat, hidden, f"{pre}{mode}0_")
        p.update(W.make_dense_weights(4, classes, 2 * hidden, f"{pre}dense0_"))
        head = WindowHead(mode, feat, hidden, classes, p, f"{pre}{mode}0_", f"{pre}dense0_", max_rows=n, max_samples=n).project(feats)
        head.forward(centre, lo, hi, T, a.stride), head.forward_rows(table)          # warm-up
        ta, tr = [], []
        for _ in range(a.runs):
            t, ref = timed(lambda: head.forward(centre, lo, hi, T, a.stride))
            ta.append(t)
            t, got = timed(lambda: head.forward_rows(table))
            tr.append(t)
        rec = dict(mode=mode, feat=feat, rows=n, window=T, stride=a.stride, forward_ms=stats(ta), forward_rows_ms=stats(tr),
                   bit_equal=bool(torch.equal(ref, got)))
        rec["rows_minus_arithmetic_ms"] = round(rec["forward_rows_ms"]["median"] - rec["forward_ms"]["median"], 3)
        print(json.dumps(rec), flush=True)
        out.append(rec)
        del head
    return out


def evaluate_routes(a):
    from tennis_amd import evaluate as ev
    out = []
    with tempfile.TemporaryDirectory() as root:
        for window in a.eval_windows:
            base = ["--root", os.path.join(root, "data"), "--exp_root", os.path.join(root, "exp"), "--frames_per_video", str(a.frames_per_video),
                    "--data_shape", "224", "--window", str(window), "--temp_pool", "gru", "--batch_size", str(a.batch_size)]
            wall, loop = {"loader": [], "dense": []}, {"loader": [], "dense": []}
            samples = None
            for _ in range(a.runs):
                for route, extra in (("loader", []), ("dense", ["--dense_windows"])):
                    buf = io.StringIO()
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    with contextlib.redirect_stdout(buf):
                        assert ev.main(base + extra) == 0
                    torch.cuda.synchronize()
                    wall[route].append(time.perf_counter() - t0)
                    m = re.search(r"# Samples: (\d+), Time Taken: ([0-9.]+)", buf.getvalue())
                    samples = int(m.group(1))
                    loop[route].append(float(m.group(2)))
            rec = dict(window=window, samples=samples, frames_encoded_loader=samples * window, batch_size=a.batch_size,
                       wall_s={k: stats(v) for k, v in wall.items()}, evaluation_loop_s={k: stats(v) for k, v in loop.items()})
            rec["wall_speedup_median"] = round(rec["wall_s"]["loader"]["median"] / rec["wall_s"]["dense"]["median"], 2)
            print(json.dumps(rec), flush=True)
            out.append(rec)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=172047)      # split-02's test frames
    ap.add_argument("--window", type=int, default=30)
    ap.add_argument("--stride", type=int, default=1)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--eval_windows", type=int, nargs="+", default=[8, 30])
    ap.add_argument("--frames_per_video", type=int, default=64)
    ap.add_argument("--batch_size", type=int, default=8)      # (the loader route's batch is batch_size x window frames)
    ap.add_argument("--out", default=os.path.join("profiles", "dense_frames_eval_bench.json"))
    a = ap.parse_args()
    doc = dict(device=torch.cuda.get_device_name(0),
               what="(a) WindowHead.forward_rows vs WindowHead.forward on the same windows, device ms; (b) evaluate on synthetic frames, "
                    "loader route vs --dense_windows, seconds; routes alternating, medians and spread (max - min) of the runs",
               head_forms=head_forms(a), evaluate=evaluate_routes(a))
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)


if __name__ == "__main__":
    main()
