"""Same-box A/B of the two matrix modes of the backbone training steps (matmul="f32" | "fp32x3", TN_MATMUL_*): one handle pair per
shape - the same parameters, the same batch - timed alternately, --reps runs of --steps (forward_backward + step) each after
--warmup, the median and the runs reported; then, in runs of their own under `rocprofv3 --kernel-trace --stats` (a fresh child
process per shape and mode; tracing slows the host, so no step time is taken there), the device time of the kernels the launch
counters count: the backbone's GEMMs and their split-K reductions.

Shapes: FrameModelTrainer at 224 x 224 x 64 and 512 x 512 x 64 frames, and the CNN-RNN step at 8 clips x 8 frames of 224 x 224.
   python scripts/bench_finetune_matmul.py [--shapes fm224,fm512,cnnrnn] [--no-profile] [--out profiles/finetune_matmul_bench.json]
The f32 columns are the baseline: the default mode calls the launchers the step always called with the same arguments, so they
must agree with the step times recorded before the mode existed (profiles/cnnrnn_train_bench.json) within the run-to-run spread;
the record says whether they do.  The mode is worth keeping where fp32x3's summed GEMM time is below f32's by more than the
spread of the runs."""
import argparse
import csv
import glob
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = {"fm224": ("frame", 224, 64, 1, 10), "fm512": ("frame", 512, 64, 1, 4), "cnnrnn": ("cnnrnn", 224, 8, 8, 10)}   # kind, side, batch, window, steps
MODES = ("f32", "fp32x3")
# the kernels behind the launch counters (linear.hip, train.hip, gemm_fp32x3.hip).  The f32 names also match the classifier's /
# the head's few launches, which no mode switches: one tiny launch per step of the frame classifier.
GEMM_KERNELS = re.compile(r"linear_f32_kernel|linear_f32_skinny_kernel|gemm_tn_f32_kernel|splitk_reduce_kernel|gemm_fp32x3_kernel")


def make(shape, mode):
    """-> (trainer, x, y, batch for step())"""
    import torch
    from tennis_amd import weights as W
    from tennis_amd.engine import CNNRNNTrainer, FrameModelTrainer
    kind, S, B, T, _ = SHAPES[shape]
    p = W.make_densenet121_weights(0)
    g = torch.Generator(device="cuda")
    g.manual_seed(1)
    x = torch.randn((B * T, S, S, 3), generator=g, device="cuda")
    y = torch.randint(0, 11, (B,), generator=g, device="cuda", dtype=torch.int32)
    if kind == "frame":
        p.update(W.make_dense_weights(1, 11, 1024, "framemodel0_dense0_"))
        return FrameModelTrainer(p, S, 11, batch=B, matmul=mode), x, y, B
    p.update(W.make_rnn_weights(2, "gru", 1024, 128, "cnnrnn0_gru0_"))
    p.update(W.make_dense_weights(1, 11, 256, "cnnrnn0_dense0_"))
    return CNNRNNTrainer(p, S, 11, batch=B, steps=T, type="gru", matmul=mode), x.view(B, T, S, S, 3), y, B


def run_steps(tr, x, y, batch, n):
    for _ in range(n):
        tr.forward_backward(x, y)
        tr.step(batch, 1e-4, 0.9, 1e-4)


def time_shape(shape, warmup, reps):
    import numpy as np
    import torch
    steps = SHAPES[shape][4]
    pair = {m: make(shape, m) for m in MODES}
    for m in MODES:
        run_steps(*pair[m], warmup)
    torch.cuda.synchronize()
    runs = {m: [] for m in MODES}
    for _ in range(reps):                         # alternating: f32, fp32x3, f32, ...
        for m in MODES:
            t0 = time.perf_counter()
            run_steps(*pair[m], steps)
            torch.cuda.synchronize()
            runs[m].append((time.perf_counter() - t0) / steps * 1e3)
    out = {}
    for m in MODES:
        f32n, x3n = pair[m][0].matmul_stats()
        out[m] = {"step_ms": round(float(np.median(runs[m])), 3), "step_ms_runs": [round(t, 3) for t in runs[m]],
                  "step_ms_spread": round(max(runs[m]) - min(runs[m]), 3),
                  "gemm_launches_per_step": (f32n + x3n) // (warmup + reps * steps), "launch_counters": [f32n, x3n]}
    del pair
    torch.cuda.synchronize()
    return out


def profile_child(shape, mode, steps):
    """what a rocprofv3 child runs: `steps` steps of one shape in one mode after one warm-up step"""
    import torch
    tr, x, y, b = make(shape, mode)
    run_steps(tr, x, y, b, 1 + steps)
    torch.cuda.synchronize()
    print("profiled", shape, mode, tr.matmul_stats(), flush=True)


def kernel_stats(outdir):
    """-> {kernel name: (calls, total ns)} from rocprofv3's kernel statistics, or summed from its kernel trace"""
    stats = {}
    files = glob.glob(os.path.join(outdir, "**", "*kernel_stats.csv"), recursive=True)
    for f in files:
        for row in csv.DictReader(open(f)):
            c, t = stats.get(row["Name"], (0, 0))
            stats[row["Name"]] = (c + int(row["Calls"]), t + int(float(row["TotalDurationNs"])))
    if not files:
        for f in glob.glob(os.path.join(outdir, "**", "*kernel_trace.csv"), recursive=True):
            for row in csv.DictReader(open(f)):
                c, t = stats.get(row["Kernel_Name"], (0, 0))
                stats[row["Kernel_Name"]] = (c + 1, t + int(row["End_Timestamp"]) - int(row["Start_Timestamp"]))
    if not stats:
        raise RuntimeError(f"no rocprofv3 kernel statistics under {outdir}")
    return stats


def profile_shape(shape, mode, steps, scratch):
    """GEMM-only device time per step: a rocprofv3 run of its own over 1 warm-up + `steps` steps"""
    outdir = os.path.join(scratch, f"prof_{shape}_{mode}")
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", outdir, "--", sys.executable, os.path.abspath(__file__),
           "--profile-child", shape, mode, "--profile-steps", str(steps)]
    log = open(os.path.join(scratch, f"prof_{shape}_{mode}.log"), "w")
    subprocess.run(cmd, check=True, stdout=log, stderr=subprocess.STDOUT, timeout=420)
    stats = kernel_stats(outdir)
    n = 1 + steps
    total = sum(t for _, t in stats.values())
    gemm = {k: v for k, v in stats.items() if GEMM_KERNELS.search(k)}
    per = [{"kernel": k, "launches_per_step": round(c / n, 2), "ms_per_step": round(t / n / 1e6, 4)}
           for k, (c, t) in sorted(gemm.items(), key=lambda kv: -kv[1][1])]
    return {"gemm_ms_per_step": round(sum(t for _, t in gemm.values()) / n / 1e6, 3),
            "gemm_launches_per_step": round(sum(c for c, _ in gemm.values()) / n, 2),
            "all_kernels_ms_per_step": round(total / n / 1e6, 3), "profiled_steps": n, "gemm_kernels": per}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="fm224,fm512,cnnrnn")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--no-profile", action="store_true", help="step times only, no rocprofv3 runs")
    ap.add_argument("--scratch", help="where rocprofv3 writes (default: a temporary directory, not kept)")
    ap.add_argument("--out", help="also write the JSON record to this file")
    ap.add_argument("--profile-child", nargs=2, metavar=("SHAPE", "MODE"), help=argparse.SUPPRESS)
    ap.add_argument("--profile-steps", type=int, default=3)
    a = ap.parse_args()
    if a.profile_child:
        return profile_child(a.profile_child[0], a.profile_child[1], a.profile_steps)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_finetune_matmul needs the GPU: there is nothing to time without one")
    own_scratch = a.scratch is None
    if own_scratch:
        a.scratch = tempfile.mkdtemp(prefix="finetune_matmul_")
    os.makedirs(a.scratch, exist_ok=True)
    res = {"device": torch.cuda.get_device_name(0), "warmup": a.warmup, "reps": a.reps, "order": "modes alternate within every rep",
           "step_ms": "host clock around `steps` x (forward_backward + step) ending in a device synchronise, per step; median of reps",
           "gemm_ms_per_step": "rocprofv3 --kernel-trace --stats in a run of its own: summed device time of the backbone GEMM kernels "
                               "and their split-K reductions, per step", "shapes": {}}
    for shape in a.shapes.split(","):
        kind, S, B, T, steps = SHAPES[shape]
        rec = {"trainer": "FrameModelTrainer" if kind == "frame" else "CNNRNNTrainer (gru, trainable)", "side": S, "batch": B, "window": T,
               "frames_per_step": B * T, "steps_per_run": steps, "modes": time_shape(shape, a.warmup, a.reps)}
        print(shape, json.dumps(rec["modes"]), flush=True)
        if not a.no_profile:
            for m in MODES:
                rec["modes"][m].update(profile_shape(shape, m, 3 if S <= 224 else 2, a.scratch))
                print(shape, m, "gemm ms/step", rec["modes"][m]["gemm_ms_per_step"], flush=True)
        f, x3 = rec["modes"]["f32"], rec["modes"]["fp32x3"]
        rec["step_speedup_fp32x3"] = round(f["step_ms"] / x3["step_ms"], 3)
        if not a.no_profile:
            rec["gemm_speedup_fp32x3"] = round(f["gemm_ms_per_step"] / x3["gemm_ms_per_step"], 3)
        res["shapes"][shape] = rec
    # the f32 columns against the record taken before the mode existed
    try:
        old = json.load(open(os.path.join(ROOT, "profiles", "cnnrnn_train_bench.json")))["runs"]
        base = {"fm224": old["framemodel_64"]["ms_per_step"], "cnnrnn": old["cnnrnn_trainable"]["ms_per_step"]}
        res["f32_baseline"] = {
            s: {"recorded_before_the_mode_ms": base[s], "f32_now_ms": res["shapes"][s]["modes"]["f32"]["step_ms"],
                "difference_ms": round(res["shapes"][s]["modes"]["f32"]["step_ms"] - base[s], 3),
                "spread_of_the_runs_ms": res["shapes"][s]["modes"]["f32"]["step_ms_spread"]}
            for s in base if s in res["shapes"]}
        res["f32_baseline"]["note"] = ("the f32 columns are the baseline: the default mode runs the launchers and arguments of the parent "
                                       "commit; recorded_before_the_mode_ms is profiles/cnnrnn_train_bench.json")
    except (OSError, KeyError):
        pass
    print(json.dumps({s: {"step_speedup_fp32x3": r["step_speedup_fp32x3"], "gemm_speedup_fp32x3": r.get("gemm_speedup_fp32x3")}
                      for s, r in res["shapes"].items()}), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)) or ".", exist_ok=True)
        json.dump(res, open(a.out, "w"), indent=1)
    if own_scratch:
        shutil.rmtree(a.scratch, ignore_errors=True)


if __name__ == "__main__":
    main()
