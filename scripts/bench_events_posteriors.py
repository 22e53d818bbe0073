"""What scoring events with HMM posteriors costs on the device, beside the host route, and that the four calls without the keyword
cost what they cost on the parent commit -> profiles/events_posteriors_bench.json.

Input and matrix: those of scripts/bench_events_transitions.py - 786 455 x 11 logits, 5 videos, a planted label sequence, the positions
a permutation of the rows, ``events.transition_scores`` of the planted labels.

  * (a) the device decode (``engine.EventDecoder.decode(transitions=T, posteriors=True)``): device time of the memcpy and the eleven
    launches (events around ``tn_event_decoder_run_posteriors``, every buffer and both workspaces allocated beforehand, ``posterior``
    NULL), and wall time of ``decode`` plus the copy-back of the events.  The path under the matrix is part of the call, so the
    forward-backward chains themselves cost the difference to ``decode(transitions=T)``.
  * (b) the host route: ``logits.cpu()`` plus ``events.hmm_posteriors(dtype=float32)``; wall time.  It is a Python loop with two
    (C, C) log-sum-exps per position, so it is timed on the FIRST VIDEO ONLY and scaled by the number of positions (the file says
    so); its posteriors of the path's labels must be the device's conf of that video within 1e-4.
  * (c) the parent-commit check of scripts/bench_events_transitions.py, by its own workers: ``decode(transitions=T)``,
    ``decode(switch_cost=2)``, ``decode(smooth=1)`` and ``decode(smooth=9)`` on this build against the parent's, device time, wall time
    and SHA-256 of every output.

One box, every run a fresh process (``--worker``), the routes alternating, three runs each; medians and the range.  This process
never opens the GPU.

    python scripts/bench_events_posteriors.py --parent-tree /path/to/parent/checkout [--out profiles/events_posteriors_bench.json]"""
import argparse
import json
import os
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from bench_events import CLASSES, ROWS, VIDEOS, _stats, make_input, summary
from bench_events_transitions import ROUTES
from bench_events_transitions import child as path_child


def worker(kind, tree, rows, reps):
    sys.path.insert(0, tree)
    import numpy as np
    import torch
    from tennis_amd.events import transition_scores
    res = {"worker": kind, "tree": tree}
    dev = torch.device("cuda")
    lab, start, perm = make_input(np, rows)
    g = torch.Generator(device=dev)
    g.manual_seed(1)
    logits = torch.randn((rows, CLASSES), generator=g, device=dev)
    inv = np.empty(rows, np.int64)
    inv[perm] = np.arange(rows)                            # position m reads row perm[m]: plant its label there
    logits[torch.arange(rows, device=dev), torch.from_numpy(lab[inv]).to(dev)] += 4.0
    one = rows // VIDEOS                                   # the positions of the first video
    trans = transition_scores(lab, start, CLASSES)
    from tennis_amd import _lib
    from tennis_amd.engine import EventDecoder
    dec = EventDecoder(rows, CLASSES)
    rows_d = torch.from_numpy(perm.astype(np.int32)).to(dev)
    start_d = torch.from_numpy(start).to(dev)
    if kind == "host":
        from tennis_amd.events import hmm_posteriors
        wall = []
        for _ in range(reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            host = logits.cpu().numpy()                    # (the whole copy, not scaled)
            t1 = time.perf_counter()
            gamma = hmm_posteriors(host, perm[:one], start[:one], trans, dtype=np.float32)
            wall.append(((t1 - t0) + (time.perf_counter() - t1) * rows / one) * 1e3)
        frames = dec.decode(logits, rows_d[:one], start_d[:one], transitions=trans, posteriors=True, return_frames=True)
        label, conf = frames["label"].cpu().numpy(), frames["conf"].cpu().numpy()
        res.update(wall=_stats(wall), timed_positions=one, scaled_by=rows / one,
                   max_abs_difference_to_device_conf=float(np.abs(gamma[np.arange(one), label].astype(np.float64) - conf).max()))
    else:
        ints = torch.empty((3, rows), dtype=torch.int32, device=dev)
        flts = torch.empty((2, rows), dtype=torch.float32, device=dev)
        count = torch.zeros(1, dtype=torch.int32, device=dev)
        P = _lib.ptr

        def launch():
            _lib.check(dec.lib.tn_event_decoder_run_posteriors(dec.handle, P(logits), rows, CLASSES, P(rows_d), P(start_d), rows, trans.ctypes.data,
                                                               None, None, None, P(ints[0]), P(ints[1]), P(ints[2]), P(flts[0]), P(flts[1]),
                                                               P(count), None), "run_posteriors")
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
            out = {k: v.cpu().numpy() for k, v in dec.decode(logits, rows_d, start_d, transitions=trans, posteriors=True).items()}
            wall.append((time.perf_counter() - t0) * 1e3)
        plain = {k: v.cpu().numpy() for k, v in dec.decode(logits, rows_d, start_d, transitions=trans).items()}
        res.update(device=_stats(devt), wall=_stats(wall), workspace_bytes=dec.workspace_bytes(), events=int(len(out["first"])),
                   same_events_as_without_the_keyword=all(np.array_equal(out[k], plain[k]) for k in ("first", "last", "cls")),
                   mean_score=float(out["score"].astype(np.float64).mean()), mean_score_without_the_keyword=float(plain["score"].astype(np.float64).mean()))
    print("RESULT " + json.dumps(res), flush=True)


def child(kind, tree, a, reps):
    cmd = [sys.executable, os.path.abspath(__file__), "--worker", kind, "--tree", tree, "--rows", str(a.rows), "--reps", str(reps)]
    env = dict(os.environ)
    env.pop("TENNIS_HIP_LIB", None)            # each tree loads its own library
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=a.child_timeout, env=env)
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
    if p.returncode != 0 or not lines:
        raise SystemExit(f"worker {kind} in {tree} failed ({p.returncode}):\n{p.stdout[-3000:]}")
    print(f"{kind} {os.path.basename(tree)}: {lines[-1][7:]}", file=sys.stderr, flush=True)
    return json.loads(lines[-1][7:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--worker", choices=["post", "host"])
    ap.add_argument("--tree", default=os.path.join(HERE, ".."))
    ap.add_argument("--parent-tree", default=None, help="a checkout of the parent commit with its library built")
    ap.add_argument("--rows", type=int, default=ROWS)
    ap.add_argument("--switch-cost", type=float, default=2.0)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-reps", type=int, default=1, help="the host route is a Python loop over every position: seconds per run")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--child-timeout", type=int, default=400)
    ap.add_argument("--out", default=os.path.join("profiles", "events_posteriors_bench.json"))
    a = ap.parse_args()
    if a.worker:
        return worker(a.worker, os.path.abspath(a.tree), a.rows, a.reps)
    this = os.path.abspath(os.path.join(HERE, ".."))
    parent = os.path.abspath(a.parent_tree) if a.parent_tree else None
    runs = {k: [] for k in ["host", "post"] + [f"{t}_{r}" for t in ("this", "parent") for r in ROUTES]}
    for _ in range(a.runs):                     # alternating, a fresh process each
        runs["host"].append(child("host", this, a, a.host_reps))
        runs["post"].append(child("post", this, a, a.reps))
        for r, (kind, w) in ROUTES.items():
            runs[f"this_{r}"].append(path_child(kind, this, a, w))
            if parent:
                runs[f"parent_{r}"].append(path_child(kind, parent, a, w))
    d, h = runs["post"], runs["host"]
    per_video = a.rows // VIDEOS
    post_ms, trans_ms = summary(d, "device")["median_ms"], summary(runs["this_trans"], "device")["median_ms"]
    doc = {"shape": {"rows": a.rows, "classes": CLASSES, "videos": VIDEOS, "runs_of": "10-200 positions", "rows_order": "permutation"},
           "matrix": "events.transition_scores of the planted labels, prior 1, scale 1",
           "switch_cost": a.switch_cost, "reps_per_run": a.reps, "host_reps_per_run": a.host_reps, "runs": a.runs,
           "posteriors": {"events": d[0]["events"], "same_events_as_without_the_keyword": all(x["same_events_as_without_the_keyword"] for x in d),
                          "mean_score": d[0]["mean_score"], "mean_score_without_the_keyword": d[0]["mean_score_without_the_keyword"],
                          "workspace_bytes": d[0]["workspace_bytes"],
                          "device_decode_device_time": summary(d, "device"), "device_decode_wall_with_copy_back": summary(d, "wall"),
                          "host_route_wall_with_logits_copy": summary(h, "wall"),
                          "host_route_timed_on": "the first video only (%d positions), scaled by %.4f" % (h[0]["timed_positions"], h[0]["scaled_by"]),
                          "host_float32_against_device_conf_first_video_max_abs": max(x["max_abs_difference_to_device_conf"] for x in h),
                          "chains_and_posterior_kernel_ms": round(post_ms - trans_ms, 4),
                          "chains_ns_per_position_of_a_video": round((post_ms - trans_ms) * 1e6 / per_video, 1)}}
    for r in ROUTES:
        cur = doc[f"{r}_this_build"] = {"device_time": summary(runs[f"this_{r}"], "device"), "wall": summary(runs[f"this_{r}"], "wall"),
                                        "events": runs[f"this_{r}"][0]["events"]}
        if parent:
            par = doc[f"{r}_parent_build"] = {"device_time": summary(runs[f"parent_{r}"], "device"),
                                              "wall": summary(runs[f"parent_{r}"], "wall"), "events": runs[f"parent_{r}"][0]["events"]}
            a_, b_ = cur["device_time"], par["device_time"]
            doc[f"{r}_device_time_difference_ms"] = round(a_["median_ms"] - b_["median_ms"], 4)
            doc[f"{r}_spread_of_three_runs_ms"] = round(max(a_["max_ms"] - a_["min_ms"], b_["max_ms"] - b_["min_ms"]), 4)
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
