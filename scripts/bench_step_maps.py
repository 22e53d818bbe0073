"""What the temporal activation maps cost, device time only -> profiles/step_maps_bench.json.

Shape: 172 047 rows as one sequence (split-02's test frames), window 30, stride 1, F = 1024, H = 128, 11 classes, GRU and LSTM, the
TABLE form (``WindowHead.forward_rows``).  Three questions:

  * off costs nothing: ``forward_rows`` without maps on this build against the PARENT commit's build (``--parent-tree``: a checkout of
    the parent commit with its library built), same box, a fresh process per run, the two alternating, three runs each; medians and
    range.  The margin is the spread of the three runs - a difference outside it is a defect, not a number to report.
  * on: ``forward_rows(..., return_tam=True)`` on this build, the same way.
  * the ``step_maps`` launch on its own at K = 256 and K = 4096, beside the max-pool launch over the same windows with and without
    its steps (``temporal_pool_rows`` at F = 4096: the launch the maps sit beside in ``TemporalPooling``).

    python scripts/bench_step_maps.py --parent-tree /path/to/parent/checkout [--out profiles/step_maps_bench.json]

Every measurement runs in a child process of its own (``--worker``); this process never opens the GPU."""
import argparse
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROWS, WINDOW, FEAT, HIDDEN, CLASSES = 172047, 30, 1024, 128, 11


def _timed(torch, fn, reps):
    """median, min, max over `reps` event-timed calls after one warm-up call, ms"""
    fn()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b))
    out.sort()
    return {"median_ms": round(out[len(out) // 2], 4), "min_ms": round(out[0], 4), "max_ms": round(out[-1], 4)}


def _table(torch, rows, window, dev):
    centre = torch.arange(rows, dtype=torch.int64, device=dev)[:, None]
    offs = (torch.arange(window, dtype=torch.int64, device=dev) - window // 2)[None, :]
    return (centre + offs).clamp_(0, rows - 1).to(torch.int32).contiguous()


def worker(kind, tree, rows, reps):
    sys.path.insert(0, tree)
    import torch
    from tennis_amd import weights as W
    dev = torch.device("cuda")
    idx = _table(torch, rows, WINDOW, dev)
    res = {"worker": kind, "tree": tree}
    if kind in ("off", "on"):
        from tennis_amd.engine import WindowHead
        g = torch.Generator(device=dev)
        g.manual_seed(FEAT)
        feats = torch.randn((rows, FEAT), generator=g, device=dev).abs_() * 0.5
        for mode in ("gru", "lstm"):
            p = W.make_rnn_weights(3, mode, FEAT, HIDDEN, f"b_{mode}0_")
            p.update(W.make_dense_weights(4, CLASSES, 2 * HIDDEN, "b_dense0_"))
            head = WindowHead(mode, FEAT, HIDDEN, CLASSES, p, f"b_{mode}0_", "b_dense0_", max_rows=rows, max_samples=rows).project(feats)
            call = (lambda: head.forward_rows(idx, return_tam=True)) if kind == "on" else (lambda: head.forward_rows(idx))
            res[mode] = _timed(torch, call, reps)
            del head
    else:
        from tennis_amd.engine import Dense, temporal_pool_rows
        for K in (256, 4096):
            g = torch.Generator(device=dev)
            g.manual_seed(K)
            pooled = torch.randn((rows, K), generator=g, device=dev)
            steps = torch.randint(0, WINDOW, (rows, K), generator=g, device=dev, dtype=torch.int32)
            dense = Dense(W.make_dense_weights(4, CLASSES, K, "b_")["b_weight"], None)
            res[f"step_maps_K{K}"] = _timed(torch, lambda: dense.step_maps(pooled, steps, WINDOW), reps)
            del pooled, steps
        g = torch.Generator(device=dev)
        g.manual_seed(1)
        x = torch.randn((rows, 4096), generator=g, device=dev)
        res["pool_rows_max_F4096"] = _timed(torch, lambda: temporal_pool_rows(x, idx, "max"), reps)
        res["pool_rows_max_steps_F4096"] = _timed(torch, lambda: temporal_pool_rows(x, idx, "max", return_steps=True), reps)
    print("RESULT " + json.dumps(res), flush=True)


def child(kind, tree, a):
    cmd = [sys.executable, os.path.abspath(__file__), "--worker", kind, "--tree", tree, "--rows", str(a.rows), "--reps", str(a.reps)]
    env = dict(os.environ)
    env.pop("TENNIS_HIP_LIB", None)            # each tree loads its own library
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=a.child_timeout, env=env)
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
    if p.returncode != 0 or not lines:
        raise SystemExit(f"worker {kind} in {tree} failed ({p.returncode}):\n{p.stdout[-3000:]}")
    return json.loads(lines[-1][7:])


def summary(runs, mode):
    v = sorted(r[mode]["median_ms"] for r in runs)
    return {"median_ms": v[len(v) // 2], "min_ms": v[0], "max_ms": v[-1], "runs_ms": [r[mode]["median_ms"] for r in runs]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--worker", choices=["off", "on", "kernel"])
    ap.add_argument("--tree", default=os.path.join(HERE, ".."))
    ap.add_argument("--parent-tree", default=None, help="a checkout of the parent commit with its library built")
    ap.add_argument("--rows", type=int, default=ROWS)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--child-timeout", type=int, default=240)
    ap.add_argument("--out", default=os.path.join("profiles", "step_maps_bench.json"))
    a = ap.parse_args()
    if a.worker:
        return worker(a.worker, os.path.abspath(a.tree), a.rows, a.reps)
    this = os.path.abspath(os.path.join(HERE, ".."))
    off_parent, off_this, on_this = [], [], []
    for _ in range(a.runs):                     # alternating, a fresh process each
        if a.parent_tree:
            off_parent.append(child("off", os.path.abspath(a.parent_tree), a))
        off_this.append(child("off", this, a))
        on_this.append(child("on", this, a))
    doc = {"shape": {"rows": a.rows, "window": WINDOW, "stride": 1, "feat": FEAT, "hidden": HIDDEN, "classes": CLASSES, "form": "table"},
           "reps_per_run": a.reps, "runs": a.runs, "kernel": child("kernel", this, a)}
    for mode in ("gru", "lstm"):
        doc[mode] = {"forward_rows_off_this_build": summary(off_this, mode), "forward_rows_with_maps": summary(on_this, mode)}
        if off_parent:
            par = doc[mode]["forward_rows_off_parent_build"] = summary(off_parent, mode)
            cur = doc[mode]["forward_rows_off_this_build"]
            spread = max(par["max_ms"] - par["min_ms"], cur["max_ms"] - cur["min_ms"])
            doc[mode]["off_difference_ms"] = round(cur["median_ms"] - par["median_ms"], 4)
            doc[mode]["spread_of_three_runs_ms"] = round(spread, 4)
            doc[mode]["off_within_spread"] = abs(cur["median_ms"] - par["median_ms"]) <= spread
        doc[mode]["maps_cost_ms"] = round(doc[mode]["forward_rows_with_maps"]["median_ms"] - doc[mode]["forward_rows_off_this_build"]["median_ms"], 4)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
