"""What decoding events with a label-switch penalty costs on the device, beside the host route -> profiles/events_viterbi_bench.json.

Input: that of scripts/bench_events.py - 786 455 x 11 logits (the 5-match corpus), 5 videos, a planted label sequence with runs of
10-200 positions (logit 4 on the planted class + standard normal noise), the positions a permutation of the rows.

  * the device decode (``engine.EventDecoder.decode(switch_cost=...)``): device time of the nine launches (events around
    ``tn_event_decoder_run_switch``, every buffer and the path workspace allocated beforehand), and wall time of ``decode`` plus the
    copy-back of the events.
  * the host route: ``logits.cpu()`` plus ``events.viterbi_labels(dtype=float32)`` and ``events.label_runs``; wall time.  Both routes
    must find the same runs.
  * the parent-commit check: ``decode(smooth=1)`` and ``decode(smooth=9)`` on this build against the parent's (``--parent-tree``: a
    checkout of the parent commit with its library built), device time and wall time as above.

One box, every run a fresh process (``--worker``), the routes alternating, three runs each; medians and the range.  This process
never opens the GPU.

    python scripts/bench_events_viterbi.py --parent-tree /path/to/parent/checkout [--out profiles/events_viterbi_bench.json]"""
import argparse
import json
import os
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from bench_events import CLASSES, ROWS, VIDEOS, _stats, make_input, summary


def worker(kind, tree, rows, reps, width, cost):
    sys.path.insert(0, tree)
    import numpy as np
    import torch
    res = {"worker": kind, "tree": tree, "width": width, "switch_cost": cost}
    dev = torch.device("cuda")
    lab, start, perm = make_input(np, rows)
    g = torch.Generator(device=dev)
    g.manual_seed(1)
    logits = torch.randn((rows, CLASSES), generator=g, device=dev)
    inv = np.empty(rows, np.int64)
    inv[perm] = np.arange(rows)                            # position m reads row perm[m]: plant its label there
    logits[torch.arange(rows, device=dev), torch.from_numpy(lab[inv]).to(dev)] += 4.0
    if kind == "host":
        from tennis_amd.events import label_runs, viterbi_labels
        wall = []
        for _ in range(reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            label = viterbi_labels(logits.cpu().numpy(), perm, start, cost, dtype=np.float32)
            first, last, cls = label_runs(label, start)
            wall.append((time.perf_counter() - t0) * 1e3)
        res["wall"] = _stats(wall)
    else:
        from tennis_amd import _lib
        from tennis_amd.engine import EventDecoder
        dec = EventDecoder(rows, CLASSES)
        rows_d = torch.from_numpy(perm.astype(np.int32)).to(dev)
        start_d = torch.from_numpy(start).to(dev)
        ints = torch.empty((3, rows), dtype=torch.int32, device=dev)
        flts = torch.empty((2, rows), dtype=torch.float32, device=dev)
        count = torch.zeros(1, dtype=torch.int32, device=dev)
        P = _lib.ptr
        head = (dec.handle, P(logits), rows, CLASSES, P(rows_d), P(start_d), rows)
        tail = (None, None, P(ints[0]), P(ints[1]), P(ints[2]), P(flts[0]), P(flts[1]), P(count), None)

        def launch():
            if kind == "path":
                _lib.check(dec.lib.tn_event_decoder_run_switch(*head, cost, *tail), "run_switch")
            else:
                _lib.check(dec.lib.tn_event_decoder_run(*head, width, *tail), "run")
        how = {"switch_cost": cost} if kind == "path" else {}
        launch()                                           # (the path workspace is allocated here)
        devt, wall = [], []
        for _ in range(reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            a.record()
            launch()
            b.record()
            torch.cuda.synchronize()
            devt.append(a.elapsed_time(b))
        for _ in range(reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = {k: v.cpu().numpy() for k, v in dec.decode(logits, rows_d, start_d, smooth=width, **how).items()}
            wall.append((time.perf_counter() - t0) * 1e3)
        res.update(device=_stats(devt), wall=_stats(wall))
        first, cls = out["first"], out["cls"]
        res["score_sum"] = float(out["score"].astype(np.float64).sum())
    res.update(events=int(len(first)), first_sum=int(first.astype(np.int64).sum()), cls_sum=int(cls.astype(np.int64).sum()))
    print("RESULT " + json.dumps(res), flush=True)


def child(kind, tree, a, width=1, reps=None):
    cmd = [sys.executable, os.path.abspath(__file__), "--worker", kind, "--tree", tree, "--rows", str(a.rows),
           "--reps", str(reps or a.reps), "--width", str(width), "--switch-cost", str(a.switch_cost)]
    env = dict(os.environ)
    env.pop("TENNIS_HIP_LIB", None)            # each tree loads its own library
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=a.child_timeout, env=env)
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
    if p.returncode != 0 or not lines:
        raise SystemExit(f"worker {kind} in {tree} failed ({p.returncode}):\n{p.stdout[-3000:]}")
    print(f"{kind} w{width} {os.path.basename(tree)}: {lines[-1][7:]}", file=sys.stderr, flush=True)
    return json.loads(lines[-1][7:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--worker", choices=["path", "smooth", "host"])
    ap.add_argument("--tree", default=os.path.join(HERE, ".."))
    ap.add_argument("--parent-tree", default=None, help="a checkout of the parent commit with its library built")
    ap.add_argument("--rows", type=int, default=ROWS)
    ap.add_argument("--width", type=int, default=1)
    ap.add_argument("--switch-cost", type=float, default=2.0)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-reps", type=int, default=1, help="the host route is a Python loop over every position: seconds per run")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--child-timeout", type=int, default=400)
    ap.add_argument("--out", default=os.path.join("profiles", "events_viterbi_bench.json"))
    a = ap.parse_args()
    if a.worker:
        return worker(a.worker, os.path.abspath(a.tree), a.rows, a.reps, a.width, a.switch_cost)
    this = os.path.abspath(os.path.join(HERE, ".."))
    parent = os.path.abspath(a.parent_tree) if a.parent_tree else None
    runs = {k: [] for k in ("path", "host", "this_w1", "this_w9", "parent_w1", "parent_w9")}
    for _ in range(a.runs):                     # alternating, a fresh process each
        runs["path"].append(child("path", this, a))
        runs["host"].append(child("host", this, a, reps=a.host_reps))
        for w in (1, 9):
            runs[f"this_w{w}"].append(child("smooth", this, a, w))
            if parent:
                runs[f"parent_w{w}"].append(child("smooth", parent, a, w))
    d, h = runs["path"], runs["host"]
    doc = {"shape": {"rows": a.rows, "classes": CLASSES, "videos": VIDEOS, "runs_of": "10-200 positions", "rows_order": "permutation"},
           "switch_cost": a.switch_cost, "reps_per_run": a.reps, "host_reps_per_run": a.host_reps, "runs": a.runs,
           "path": {"events_device": d[0]["events"], "events_host": h[0]["events"], "events_width_1": runs["this_w1"][0]["events"],
                    "same_events": all(d[0][k] == h[0][k] for k in ("events", "first_sum", "cls_sum")),
                    "device_decode_device_time": summary(d, "device"), "device_decode_wall_with_copy_back": summary(d, "wall"),
                    "host_route_wall_with_logits_copy": summary(h, "wall")}}
    for w in (1, 9):
        cur = doc[f"smooth_{w}_this_build"] = {"device_time": summary(runs[f"this_w{w}"], "device"), "wall": summary(runs[f"this_w{w}"], "wall"),
                                               "events": runs[f"this_w{w}"][0]["events"]}
        if parent:
            par = doc[f"smooth_{w}_parent_build"] = {"device_time": summary(runs[f"parent_w{w}"], "device"),
                                                     "wall": summary(runs[f"parent_w{w}"], "wall"), "events": runs[f"parent_w{w}"][0]["events"]}
            a_, b_ = cur["device_time"], par["device_time"]
            spread = max(a_["max_ms"] - a_["min_ms"], b_["max_ms"] - b_["min_ms"])
            doc[f"smooth_{w}_device_time_difference_ms"] = round(a_["median_ms"] - b_["median_ms"], 4)
            doc[f"smooth_{w}_spread_of_three_runs_ms"] = round(spread, 4)
            doc[f"smooth_{w}_same_result"] = all(runs[f"this_w{w}"][0][k] == runs[f"parent_w{w}"][0][k]
                                                 for k in ("events", "first_sum", "cls_sum", "score_sum"))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
