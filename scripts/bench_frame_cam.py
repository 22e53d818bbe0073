"""What the class activation maps of the frame classifier cost, and that not asking for them costs nothing
(tn_densenet121_forward_class_maps, csrc/class_maps.hip).  Default conversion, seeded weights, uint8 frames, Dense(11), B = 256:
  (a) ``forward`` WITHOUT maps on this build and - with --parent_lib - on the parent commit's build (the figure asked for: 224 x 224);
  (b) the cost of the maps ON, at 224 x 224 and at 512 x 512, in ms per call and as a share of the call;
  (c) from ``tn_dbg_profile_class_maps`` (HIP events around every launch, one stream), the new kernel's time beside
      ``head_bnrelu_avgpool7``'s, which reads the same map once.
Same box; every run is a fresh process (one library per process), this build and the parent's alternating, --reps runs each;
medians, spread and every run are kept.  The one requirement: "off" on this build equals "off" on the parent's within the
spread of the runs (``off_equals_parent``).  The cost of "on" has no bar.
  python scripts/bench_frame_cam.py [--parent_lib parent/libtennis_hip.so] [--out profiles/frame_cam_bench.json]"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

CLASSES = 11


def summary(ts, digits=4):
    return {"median": round(float(np.median(ts)), digits), "min": round(min(ts), digits), "max": round(max(ts), digits),
            "spread": round(max(ts) - min(ts), digits), "runs": [round(t, digits) for t in ts]}


def device_ms(fn, calls):
    """ms per call between two events on the current stream, the calls back to back"""
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / calls


def one_run(sizes, batch, calls, warmup):
    """one process' measurement: {size: {off, on (ms per call), class_maps_ms, head_ms (profiled, per launch)}}; "on" only where the
    library has it"""
    import ctypes
    import torch
    from tennis_amd import _lib
    have = ctypes.CDLL(_lib.LIB_PATH)
    for name in [n for n in _lib._SIGS if not hasattr(have, n)]:        # a library without the newer entry points: bind what it has
        del _lib._SIGS[name]
    has_on = hasattr(have, "tn_densenet121_forward_class_maps")
    from tennis_amd import weights as W
    from tennis_amd.engine import Dense, DenseNet121Features
    p = W.make_densenet121_weights(0)
    out = {}
    for size in sizes:
        enc = DenseNet121Features(p, size, max_batch=batch)
        d = W.make_dense_weights(1, CLASSES, enc.feature_dim, "framemodel0_dense0_")
        cls = Dense(d["framemodel0_dense0_weight"], d["framemodel0_dense0_bias"])
        g = torch.Generator(device="cuda")
        g.manual_seed(size)
        x = torch.randint(0, 256, (batch, size, size, 3), generator=g, device="cuda", dtype=torch.uint8)
        feat = torch.empty((batch, enc.feature_dim), dtype=torch.float32, device="cuda")

        def off():
            enc(x, out=feat)

        def on():
            enc(x, out=feat, class_maps=cls)

        # The same sequence of work on every build: 2 x warmup forwards, then four windows off, on, off, on.  A library without the
        # maps runs "off" in the "on" slots as well, and those windows are dropped: its "off" windows then sit at the same distance
        # from the start of the process as this build's (the chip is still raising its clocks over the first tens of ms of work:
        # with three warm-up forwards and two back-to-back windows the parent came out 1.3 - 1.6 % slower at 224 x 224 than this
        # build, with every kernel family equally fast on both under the profiler).
        modes = (("off", off), ("on", on if has_on else off))
        for _ in range(warmup):
            for _, fn in modes:
                fn()
        row = {"feature_dim": int(enc.feature_dim)}
        for key, fn in modes * 2:
            row.setdefault(key + "_windows", []).append(device_ms(fn, calls))
        for key, _ in modes if has_on else modes[:1]:
            row[key] = float(np.mean(row[key + "_windows"]))
        fams = {}
        for _ in range(3):                                              # per kernel family, one stream (both builds have this)
            for st in enc.profile(x)[0]:
                fams.setdefault(st["name"], []).append(st["ms"])
        row["families_ms"] = {n: float(np.median(v)) for n, v in fams.items()}
        if has_on:
            cm, hd = [], []
            for _ in range(3):
                stats, _, maps = enc.profile_class_maps(x, cls)
                by = {s["name"]: s for s in stats}
                cm.append(by["class_maps"]["ms"])
                hd.append(by["head_bnrelu_avgpool7"]["ms"])
            row["class_maps_ms"], row["head_ms"] = float(np.median(cm)), float(np.median(hd))
            row["map_bytes"] = int(by["head_bnrelu_avgpool7"]["bytes"] - batch * enc.feature_dim * 4)
            row["maps_shape"] = list(maps.shape)
        out[str(size)] = row
        del enc
        torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=50, help="timed forwards per window (two windows per mode and run)")
    ap.add_argument("--warmup", type=int, default=25, help="warm-up forwards per mode and size")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--sizes", default="224,512")
    ap.add_argument("--parent_lib", default=None, help="libtennis_hip.so of the parent commit: its forward is timed in alternation")
    ap.add_argument("--child", action="store_true", help="(a run's process) print the run's figures only")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "frame_cam_bench.json"))
    a = ap.parse_args()
    sizes = [int(s) for s in a.sizes.split(",")]
    if a.child:
        print(json.dumps(one_run(sizes, a.batch, a.calls, a.warmup)))
        return
    import torch
    assert torch.cuda.is_available(), "bench_frame_cam needs the GPU: there is nothing to time without it"
    base = [sys.executable, os.path.abspath(__file__), "--child", "--calls", str(a.calls), "--warmup", str(a.warmup), "--batch", str(a.batch)]
    builds = {"this": None, "parent": os.path.abspath(a.parent_lib) if a.parent_lib else None}
    runs = {b: [] for b in builds if b == "this" or builds[b]}
    for rep in range(a.reps):                                          # alternating, a fresh process per run
        # both builds run the same sizes and take turns at going first
        for b in (list(runs) if rep % 2 == 0 else list(runs)[::-1]):
            env = dict(os.environ, TENNIS_HIP_LIB=builds[b]) if builds[b] else dict(os.environ)
            cmd = base + ["--sizes", a.sizes]
            out = subprocess.run(cmd, env=env, check=True, capture_output=True, text=True, timeout=600).stdout.strip().splitlines()[-1]
            print(b, rep, out, flush=True)
            runs[b].append(json.loads(out))
    rows = []
    for size in sizes:
        k = str(size)
        first = runs["this"][0][k]
        row = {"size": size, "batch": a.batch, "classes": CLASSES, "feature_dim": first["feature_dim"], "maps_shape": first["maps_shape"],
               "map_bytes": first["map_bytes"], "timed_calls_per_window": a.calls}
        for key in ("off", "on"):
            row["forward_maps_%s_ms" % key] = summary([r[k][key] for r in runs["this"]])
        off, on = row["forward_maps_off_ms"], row["forward_maps_on_ms"]
        row["cost_of_maps_ms"] = round(on["median"] - off["median"], 4)
        row["cost_of_maps_percent_of_call"] = round(100.0 * (on["median"] - off["median"]) / on["median"], 2)
        cm, hd = summary([r[k]["class_maps_ms"] for r in runs["this"]]), summary([r[k]["head_ms"] for r in runs["this"]])
        row["profiled_class_maps_kernel_ms"], row["profiled_head_kernel_ms"] = cm, hd
        row["class_maps_over_head"] = round(cm["median"] / hd["median"], 2)
        row["class_maps_map_read_GBps"] = round(row["map_bytes"] / (cm["median"] * 1e-3) / 1e9, 1)
        if "parent" in runs:
            par = summary([r[k]["off"] for r in runs["parent"]])
            row["forward_parent_ms"] = par
            row["off_minus_parent_ms"] = round(off["median"] - par["median"], 4)          # negative: this build is faster
            row["off_equals_parent"] = bool(abs(off["median"] - par["median"]) <= max(off["spread"], par["spread"]))
            row["off_not_slower_than_parent"] = bool(off["median"] - par["median"] <= max(off["spread"], par["spread"]))
            # where a difference sits: the profiled time of every kernel family, this build minus the parent's (medians over the runs)
            fam = lambda rs, n: float(np.median([r[k]["families_ms"][n] for r in rs]))
            row["families_this_minus_parent_ms"] = {n: round(fam(runs["this"], n) - fam(runs["parent"], n), 4) for n in runs["parent"][0][k]["families_ms"]}
            row["families_parent_ms"] = {n: round(fam(runs["parent"], n), 4) for n in runs["parent"][0][k]["families_ms"]}
        rows.append(row)
        print(json.dumps(row), flush=True)
    res = {"device": torch.cuda.get_device_name(0),
           "what": "DenseNet121Features forward (default conversion, seeded weights, uint8 frames, B = %d), class activation maps of a Dense(%d) "
                   "off and on: device ms per call; the new kernel beside head_bnrelu_avgpool7 under tn_dbg_profile_class_maps (HIP events, "
                   "one stream); every run a fresh process, this build and the parent's alternating" % (a.batch, CLASSES),
           "reps": a.reps, "rows": rows, "parent_build": "timed" if "parent" in runs else "NOT MEASURED in this run (no --parent_lib)"}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
