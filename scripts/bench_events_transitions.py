"""What decoding events under a class-transition matrix costs on the device, beside the host route and beside the switch-cost path
-> profiles/events_transitions_bench.json.

Input: that of scripts/bench_events.py - 786 455 x 11 logits (the 5-match corpus), 5 videos, a planted label sequence with runs of
10-200 positions (logit 4 on the planted class + standard normal noise), the positions a permutation of the rows.  The matrix is
``events.transition_scores`` of the planted label sequence (prior 1, scale 1).

  * (a) the device decode (``engine.EventDecoder.decode(transitions=T)``): device time of the memcpy and the nine launches (events
    around ``tn_event_decoder_run_transitions``, every buffer and the back-pointer workspace allocated beforehand), and wall time of
    ``decode`` plus the copy-back of the events.
  * (b) the host route: ``logits.cpu()`` plus ``events.viterbi_labels(dtype=float32, transitions=T)`` and ``events.label_runs``; wall
    time.  It is a Python loop with a (C, C) sum per position, so it is timed on the FIRST VIDEO ONLY and scaled by the number of
    positions (the file says so); the runs it finds there must be the device's runs of that video (count, sum of the first
    positions, sum of the classes).
  * (c) the parent-commit check: ``decode(transitions=T)``, ``decode(switch_cost=2)``, ``decode(smooth=1)`` and ``decode(smooth=9)``
    on this build against the parent's (``--parent-tree``: a checkout of the parent commit with its library built), device time and
    wall time as above, and a SHA-256 of the bytes of ``label``, ``conf`` and the five event arrays: the two builds must agree on
    every one, and this build's median device time is held against the parent's own range over its runs, widened by its width.
  * (d) the per-position time of the two chains: device time over the positions of one video (the videos run side by side).

One box, every run a fresh process (``--worker``), the routes alternating, three runs each; medians and the range.  This process
never opens the GPU.

    python scripts/bench_events_transitions.py --parent-tree /path/to/parent/checkout [--out profiles/events_transitions_bench.json]"""
import argparse
import hashlib
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
    one = rows // VIDEOS                                   # the positions of the first video
    if kind in ("trans", "host"):
        from tennis_amd.events import transition_scores
        trans = transition_scores(lab, start, CLASSES)
        res["transitions_min_diagonal"] = float(np.diagonal(trans).min())
        res["transitions_max_off_diagonal"] = float(trans[~np.eye(CLASSES, dtype=bool)].max())
    if kind == "host":
        from tennis_amd.events import label_runs, viterbi_labels
        wall = []
        for _ in range(reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            host = logits.cpu().numpy()                    # (the whole copy, not scaled)
            t1 = time.perf_counter()
            label = viterbi_labels(host, perm[:one], start[:one], dtype=np.float32, transitions=trans)
            first, last, cls = label_runs(label, start[:one])
            wall.append(((t1 - t0) + (time.perf_counter() - t1) * rows / one) * 1e3)
        res.update(wall=_stats(wall), timed_positions=one, scaled_by=rows / one)
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
            if kind == "trans":
                _lib.check(dec.lib.tn_event_decoder_run_transitions(*head, trans.ctypes.data, *tail), "run_transitions")
            elif kind == "path":
                _lib.check(dec.lib.tn_event_decoder_run_switch(*head, cost, *tail), "run_switch")
            else:
                _lib.check(dec.lib.tn_event_decoder_run(*head, width, *tail), "run")
        how = {"transitions": trans} if kind == "trans" else {"switch_cost": cost} if kind == "path" else {}
        launch()                                           # (the workspaces are allocated here)
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
        res.update(device=_stats(devt), wall=_stats(wall), workspace_bytes=dec.workspace_bytes())
        frames = dec.decode(logits, rows_d, start_d, smooth=width, return_frames=True, **how)
        res["sha256"] = {k: hashlib.sha256(v.cpu().numpy().tobytes()).hexdigest() for k, v in sorted(frames.items())}
        first, cls = out["first"], out["cls"]
        res["score_sum"] = float(out["score"].astype(np.float64).sum())
        res.update(events_all=int(len(first)), first_sum_all=int(first.astype(np.int64).sum()), cls_sum_all=int(cls.astype(np.int64).sum()))
        if kind == "trans":                                # what the host route is compared with: the first video's events
            first, cls = first[out["first"] < one], cls[out["first"] < one]
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


ROUTES = {"trans": ("trans", 1), "cost": ("path", 1), "w1": ("smooth", 1), "w9": ("smooth", 9)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--worker", choices=["trans", "path", "smooth", "host"])
    ap.add_argument("--tree", default=os.path.join(HERE, ".."))
    ap.add_argument("--parent-tree", default=None, help="a checkout of the parent commit with its library built")
    ap.add_argument("--rows", type=int, default=ROWS)
    ap.add_argument("--width", type=int, default=1)
    ap.add_argument("--switch-cost", type=float, default=2.0)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-reps", type=int, default=1, help="the host route is a Python loop over every position: seconds per run")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--child-timeout", type=int, default=400)
    ap.add_argument("--out", default=os.path.join("profiles", "events_transitions_bench.json"))
    a = ap.parse_args()
    if a.worker:
        return worker(a.worker, os.path.abspath(a.tree), a.rows, a.reps, a.width, a.switch_cost)
    this = os.path.abspath(os.path.join(HERE, ".."))
    parent = os.path.abspath(a.parent_tree) if a.parent_tree else None
    runs = {k: [] for k in ["host"] + [f"{t}_{r}" for t in ("this", "parent") for r in ROUTES]}
    for _ in range(a.runs):                     # alternating, a fresh process each
        runs["host"].append(child("host", this, a, reps=a.host_reps))
        for r, (kind, w) in ROUTES.items():
            runs[f"this_{r}"].append(child(kind, this, a, w))
            if parent:
                runs[f"parent_{r}"].append(child(kind, parent, a, w))
    d, h = runs["this_trans"], runs["host"]
    per_video = a.rows // VIDEOS
    doc = {"shape": {"rows": a.rows, "classes": CLASSES, "videos": VIDEOS, "runs_of": "10-200 positions", "rows_order": "permutation"},
           "matrix": {"from": "events.transition_scores of the planted labels, prior 1, scale 1",
                      "min_diagonal": d[0]["transitions_min_diagonal"], "max_off_diagonal": d[0]["transitions_max_off_diagonal"]},
           "switch_cost": a.switch_cost, "reps_per_run": a.reps, "host_reps_per_run": a.host_reps, "runs": a.runs,
           "transitions": {"events_device": d[0]["events_all"], "events_switch_cost": runs["this_cost"][0]["events"],
                           "events_width_1": runs["this_w1"][0]["events"], "workspace_bytes": d[0]["workspace_bytes"],
                           "device_decode_device_time": summary(d, "device"), "device_decode_wall_with_copy_back": summary(d, "wall"),
                           "host_route_wall_with_logits_copy": summary(h, "wall"),
                           "host_route_timed_on": "the first video only (%d positions), scaled by %.4f" % (h[0]["timed_positions"], h[0]["scaled_by"]),
                           "events_first_video_device": d[0]["events"], "events_first_video_host": h[0]["events"],
                           "same_events_first_video": all(d[0][k] == h[0][k] for k in ("events", "first_sum", "cls_sum"))}}
    chain = {"transitions": summary(d, "device")["median_ms"], "switch_cost": summary(runs["this_cost"], "device")["median_ms"]}
    doc["ns_per_position_of_a_video"] = {k: round(v * 1e6 / per_video, 1) for k, v in chain.items()}
    for r in ROUTES:
        cur = doc[f"{r}_this_build"] = {"device_time": summary(runs[f"this_{r}"], "device"), "wall": summary(runs[f"this_{r}"], "wall"),
                                        "events": runs[f"this_{r}"][0]["events"]}
        if parent:
            par = doc[f"{r}_parent_build"] = {"device_time": summary(runs[f"parent_{r}"], "device"),
                                              "wall": summary(runs[f"parent_{r}"], "wall"), "events": runs[f"parent_{r}"][0]["events"]}
            a_, b_ = cur["device_time"], par["device_time"]
            spread = max(a_["max_ms"] - a_["min_ms"], b_["max_ms"] - b_["min_ms"])
            doc[f"{r}_device_time_difference_ms"] = round(a_["median_ms"] - b_["median_ms"], 4)
            doc[f"{r}_spread_of_three_runs_ms"] = round(spread, 4)
            doc[f"{r}_same_result"] = all(runs[f"this_{r}"][0][k] == runs[f"parent_{r}"][0][k]
                                          for k in ("events_all", "first_sum_all", "cls_sum_all", "score_sum"))
            doc[f"{r}_sha256"] = runs[f"parent_{r}"][0]["sha256"]
            doc[f"{r}_same_sha256"] = all(x["sha256"] == doc[f"{r}_sha256"] for x in runs[f"this_{r}"] + runs[f"parent_{r}"])
            width = b_["max_ms"] - b_["min_ms"]
            doc[f"{r}_median_inside_parent_range_widened_by_its_width"] = b_["min_ms"] - width <= a_["median_ms"] <= b_["max_ms"] + width
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
