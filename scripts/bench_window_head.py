"""Dense windowed evaluation of the temporal head against the sample-by-sample path, device time only.

Baseline (the path without this feature, same handle types): torch index-gather of the windows from the device-resident feature
matrix -> ``CNNRNN.forward`` in batches of 256.  Dense: ``WindowHead.project`` once, ``WindowHead.forward`` once.  The two
alternate, three runs each; project and forward are timed separately; the rows-per-workgroup forms of the recurrent kernel are
timed as well.  One JSON document -> profiles/window_head_bench.json.

    python scripts/bench_window_head.py [--rows 172047] [--window 30] [--feats 1024 4096] [--out profiles/window_head_bench.json]
"""
import argparse
import json
import os
import sys

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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=172047)      # split-02's test frames
    ap.add_argument("--window", type=int, default=30)
    ap.add_argument("--stride", type=int, default=1)
    ap.add_argument("--feats", type=int, nargs="+", default=[1024, 4096])
    ap.add_argument("--modes", nargs="+", default=["gru", "lstm"])
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--out", default=os.path.join("profiles", "window_head_bench.json"))
    a = ap.parse_args()
    from tennis_amd import weights as W
    from tennis_amd.engine import WindowHead
    from tennis_amd.models.vision.definitions import CNNRNN
    n, T, hidden, classes = a.rows, a.window, 128, 11
    dev = torch.device("cuda")
    centre = torch.arange(n, dtype=torch.int32, device=dev)
    lo, hi = torch.zeros_like(centre), torch.full_like(centre, n - 1)
    offs = (torch.arange(T, device=dev) - T // 2) * a.stride
    results = []
    for feat in a.feats:
        g = torch.Generator(device=dev)
        g.manual_seed(feat)
        feats = torch.randn((n, feat), generator=g, device=dev).abs_() * 0.5
        for mode in a.modes:
            pre = f"bench_{mode}{feat}_"
            m = CNNRNN(None, num_classes=classes, type=mode, hidden_size=hidden, prefix=pre)
            m.initialize()
            p = W.make_rnn_weights(3, mode, feat, hidden, f"{pre}{mode}0_")
            p.update(W.make_dense_weights(4, classes, 2 * hidden, f"{pre}dense0_"))
            m.set_params(p)
            head = WindowHead(mode, feat, hidden, classes, p, f"{pre}{mode}0_", f"{pre}dense0_", max_rows=n, max_samples=n)

            def baseline():
                out = torch.empty((n, classes), device=dev)
                for s in range(0, n, a.batch):
                    idx = (centre[s:s + a.batch, None].long() + offs[None, :]).clamp_(0, n - 1)
                    out[s:s + a.batch] = m(feats[idx])
                return out

            head.project(feats).forward(centre, lo, hi, T, a.stride)      # warm-up of both paths (handles, workspaces)
            m(feats[:a.batch * T].view(a.batch, T, feat))
            rec = dict(mode=mode, feat=feat, rows=n, window=T, stride=a.stride, batch=a.batch, baseline_ms=[], project_ms=[], forward_ms=[])
            for _ in range(a.runs):
                tb, ref = timed(baseline)
                tp, _ = timed(lambda: head.project(feats))
                tf, got = timed(lambda: head.forward(centre, lo, hi, T, a.stride))
                rec["baseline_ms"].append(round(tb, 3)); rec["project_ms"].append(round(tp, 3)); rec["forward_ms"].append(round(tf, 3))
            rec["max_abs_diff_vs_baseline"] = float((ref - got).abs().max().item())
            for nb in (4, 6 if mode == "gru" else 8):
                head._set_rows_per_group(nb)
                rec[f"forward_ms_rows_per_group_{nb}"] = [round(timed(lambda: head.forward(centre, lo, hi, T, a.stride))[0], 3) for _ in range(a.runs)]
            head._set_rows_per_group(0)
            med = lambda v: float(np.median(v))
            rec["speedup_median"] = round(med(rec["baseline_ms"]) / (med(rec["project_ms"]) + med(rec["forward_ms"])), 2)
            print(json.dumps(rec), flush=True)
            results.append(rec)
            del head, m
        del feats
        torch.cuda.empty_cache()
    doc = dict(device=torch.cuda.get_device_name(0), what="dense windowed evaluation vs index-gather + CNNRNN.forward, device ms", results=results)
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)


if __name__ == "__main__":
    main()
