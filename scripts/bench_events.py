"""What decoding events on the device costs, beside the host route it replaces -> profiles/events_bench.json.

Input: 786 455 x 11 logits (the 5-match corpus), 5 videos, a planted label sequence with runs of 10-200 positions (logit 4 on the
planted class + standard normal noise), the positions a permutation of the rows.

  * route A, the device decode (``engine.EventDecoder``) at width 1 and 9: device time of the four launches (events around
    ``tn_event_decoder_run`` with every buffer allocated beforehand), and wall time of ``decode`` plus the copy-back of the events.
  * route B, the same result the way it had to be done before: ``logits.cpu()`` plus a float32 numpy restatement of the definitions
    (below, in this script: it imports nothing of ``oracle/`` or ``tests/``); wall time.
  * the parent-commit check: ``evaluate --dense_windows`` WITHOUT ``--save_events`` on the synthetic split, this build against the
    parent's (``--parent-tree``: a checkout of the parent commit with its library built), wall time of ``main``.  The difference must lie
    inside the spread of the three runs.

One box, every run a fresh process (``--worker``), the routes alternating, three runs each; medians and the spread.  This process
never opens the GPU.

    python scripts/bench_events.py --parent-tree /path/to/parent/checkout [--out profiles/events_bench.json]"""
import argparse
import json
import os
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROWS, CLASSES, VIDEOS = 786455, 11, 5
EVAL_ARGS = ["--frames_per_video", "64", "--data_shape", "224", "--window", "4", "--stride", "2", "--temp_pool", "gru", "--batch_size", "16",
             "--dense_windows"]


def make_input(np, rows, seed=0):
    """-> (labels (rows,) planted, start (rows,), perm (rows,)): runs of 10-200 positions, VIDEOS videos of equal length"""
    rng = np.random.default_rng(seed)
    lens = rng.integers(10, 201, rows // 10 + 1)
    lab = np.repeat(rng.integers(0, CLASSES, len(lens)), lens)[:rows]
    start = np.zeros(rows, np.int32)
    start[[v * (rows // VIDEOS) for v in range(VIDEOS)]] = 1
    return lab, start, rng.permutation(rows)


def decode_host(np, logits, rows, start, width):
    """The definitions of include/tennis_hip.h in float32 numpy -> (first, last, cls, score, peak)."""
    x = logits[np.clip(rows, 0, len(logits) - 1)]
    e = np.exp(x - x.max(1, keepdims=True))
    p = e / e.sum(1, keepdims=True, dtype=np.float32)
    m, h = len(p), (width - 1) // 2
    begins = start != 0
    begins[0] = True
    if h:
        vid = np.cumsum(begins) - 1
        acc, cnt = p.copy(), np.ones(m, np.float32)
        for d in range(1, h + 1):                          # (not the kernel's order of additions: the same sum up to rounding)
            ok = vid[d:] == vid[:-d]
            acc[d:] += p[:-d] * ok[:, None]
            acc[:-d] += p[d:] * ok[:, None]
            cnt[d:] += ok
            cnt[:-d] += ok
        p = acc / cnt[:, None]
    label = p.argmax(1)
    conf = p[np.arange(m), label]
    run = begins.copy()
    run[1:] |= label[1:] != label[:-1]
    first = np.flatnonzero(run)
    last = np.append(first[1:], m) - 1
    score = np.add.reduceat(conf, first, dtype=np.float32) / (last - first + 1).astype(np.float32)
    return first, last, label[first], score, np.maximum.reduceat(conf, first)


def _stats(v):
    v = sorted(v)
    return {"median_ms": round(v[len(v) // 2], 4), "min_ms": round(v[0], 4), "max_ms": round(v[-1], 4)}


def worker(kind, tree, rows, reps, width):
    sys.path.insert(0, tree)
    import numpy as np
    import torch
    res = {"worker": kind, "tree": tree, "width": width}
    if kind == "evaluate":
        import contextlib
        import io
        import tempfile
        from tennis_amd import evaluate as ev
        with tempfile.TemporaryDirectory() as tmp:
            args = ["--root", os.path.join(tmp, "data"), "--exp_root", os.path.join(tmp, "exp")] + EVAL_ARGS
            times = []
            for i in range(reps + 1):                      # the first call builds the engines: warm-up
                buf = io.StringIO()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                with contextlib.redirect_stdout(buf):
                    assert ev.main(args) == 0
                torch.cuda.synchronize()
                if i:
                    times.append((time.perf_counter() - t0) * 1e3)
            res["wall"] = _stats(times)
            res["finished"] = [ln for ln in buf.getvalue().splitlines() if ln.startswith("[Finished]")][0].split("  #")[0]
        print("RESULT " + json.dumps(res), flush=True)
        return
    dev = torch.device("cuda")
    lab, start, perm = make_input(np, rows)
    g = torch.Generator(device=dev)
    g.manual_seed(1)
    logits = torch.randn((rows, CLASSES), generator=g, device=dev)
    inv = np.empty(rows, np.int64)
    inv[perm] = np.arange(rows)                            # position m reads row perm[m]: plant its label there
    logits[torch.arange(rows, device=dev), torch.from_numpy(lab[inv]).to(dev)] += 4.0
    if kind == "device":
        from tennis_amd import _lib
        from tennis_amd.engine import EventDecoder
        dec = EventDecoder(rows, CLASSES)
        rows_d = torch.from_numpy(perm.astype(np.int32)).to(dev)
        start_d = torch.from_numpy(start).to(dev)
        ints = torch.empty((3, rows), dtype=torch.int32, device=dev)
        flts = torch.empty((2, rows), dtype=torch.float32, device=dev)
        count = torch.zeros(1, dtype=torch.int32, device=dev)
        P = _lib.ptr

        def launch():
            _lib.check(dec.lib.tn_event_decoder_run(dec.handle, P(logits), rows, CLASSES, P(rows_d), P(start_d), rows, width, None, None,
                                                    P(ints[0]), P(ints[1]), P(ints[2]), P(flts[0]), P(flts[1]), P(count), None), "run")
        launch()
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
            out = {k: v.cpu().numpy() for k, v in dec.decode(logits, rows_d, start_d, smooth=width).items()}
            wall.append((time.perf_counter() - t0) * 1e3)
        res.update(device=_stats(devt), wall=_stats(wall))
        first, score = out["first"], out["score"]
    else:
        wall = []
        for _ in range(reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            first, last, cls, score, peak = decode_host(np, logits.cpu().numpy(), perm, start, width)
            wall.append((time.perf_counter() - t0) * 1e3)
        res["wall"] = _stats(wall)
    res.update(events=int(len(first)), first_sum=int(first.astype(np.int64).sum()), score_sum=float(score.astype(np.float64).sum()))
    print("RESULT " + json.dumps(res), flush=True)


def child(kind, tree, a, width=1):
    cmd = [sys.executable, os.path.abspath(__file__), "--worker", kind, "--tree", tree, "--rows", str(a.rows), "--reps", str(a.reps),
           "--width", str(width)]
    env = dict(os.environ)
    env.pop("TENNIS_HIP_LIB", None)            # each tree loads its own library
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=a.child_timeout, env=env)
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
    if p.returncode != 0 or not lines:
        raise SystemExit(f"worker {kind} in {tree} failed ({p.returncode}):\n{p.stdout[-3000:]}")
    return json.loads(lines[-1][7:])


def summary(runs, key):
    v = sorted(r[key]["median_ms"] for r in runs)
    return {"median_ms": v[len(v) // 2], "min_ms": v[0], "max_ms": v[-1], "runs_ms": [r[key]["median_ms"] for r in runs]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--worker", choices=["device", "host", "evaluate"])
    ap.add_argument("--tree", default=os.path.join(HERE, ".."))
    ap.add_argument("--parent-tree", default=None, help="a checkout of the parent commit with its library built")
    ap.add_argument("--rows", type=int, default=ROWS)
    ap.add_argument("--width", type=int, default=1)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--child-timeout", type=int, default=240)
    ap.add_argument("--out", default=os.path.join("profiles", "events_bench.json"))
    a = ap.parse_args()
    if a.worker:
        return worker(a.worker, os.path.abspath(a.tree), a.rows, a.reps, a.width)
    this = os.path.abspath(os.path.join(HERE, ".."))
    runs = {k: [] for k in ("device_w1", "device_w9", "host_w1", "host_w9", "eval_parent", "eval_this")}
    for _ in range(a.runs):                     # alternating, a fresh process each
        for w in (1, 9):
            runs[f"device_w{w}"].append(child("device", this, a, w))
            runs[f"host_w{w}"].append(child("host", this, a, w))
        if a.parent_tree:
            runs["eval_parent"].append(child("evaluate", os.path.abspath(a.parent_tree), a))
        runs["eval_this"].append(child("evaluate", this, a))
    doc = {"shape": {"rows": a.rows, "classes": CLASSES, "videos": VIDEOS, "runs_of": "10-200 positions", "rows_order": "permutation"},
           "reps_per_run": a.reps, "runs": a.runs}
    for w in (1, 9):
        d, h = runs[f"device_w{w}"], runs[f"host_w{w}"]
        doc[f"width_{w}"] = {"events_device": d[0]["events"], "events_host": h[0]["events"],
                             "same_events": d[0]["events"] == h[0]["events"] and d[0]["first_sum"] == h[0]["first_sum"],
                             "score_sum_device": d[0]["score_sum"], "score_sum_host": h[0]["score_sum"],
                             "device_decode_device_time": summary(d, "device"), "device_decode_wall_with_copy_back": summary(d, "wall"),
                             "host_route_wall_with_logits_copy": summary(h, "wall")}
    cur = doc["evaluate_dense_windows_without_the_flag_this_build"] = dict(summary(runs["eval_this"], "wall"), args=EVAL_ARGS,
                                                                          finished=runs["eval_this"][0]["finished"])
    if runs["eval_parent"]:
        par = doc["evaluate_dense_windows_parent_build"] = dict(summary(runs["eval_parent"], "wall"), finished=runs["eval_parent"][0]["finished"])
        spread = max(par["max_ms"] - par["min_ms"], cur["max_ms"] - cur["min_ms"])
        doc["evaluate_difference_ms"] = round(cur["median_ms"] - par["median_ms"], 4)
        doc["spread_of_three_runs_ms"] = round(spread, 4)
        doc["evaluate_within_spread"] = abs(cur["median_ms"] - par["median_ms"]) <= spread
        doc["evaluate_same_scores"] = cur["finished"] == par["finished"]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
