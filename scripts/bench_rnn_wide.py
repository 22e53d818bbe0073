"""The wide recurrent kernels (csrc/rnn.hip rnn_recurrent_wide_kernel, csrc/rnn_bptt.hip rnn_bptt_wide_kernel: two gate rows per thread,
1024 < gates*H <= 2048) at config C5's shapes (32 clips x 214 steps x 1024 features, E = 100, V = 254, 20-token captions, beam 5),
H = 512 beside H = 256, which runs the kernels it always ran.  Same box, the widths alternating, --reps runs each; medians and every
run are kept.  No parent-commit number exists for H = 512: the parent refuses the shape.
  (a) the captioner's training step (forward_backward + Adam step), device ms per step, GRU and LSTM, H = 256 and 512;
  (b) encode + beam search (150 decoding steps), device ms per call, the same four;
      with --parent_lib PATH the H = 256 rows of (a) and (b) are ALSO timed in a child process on that library (the parent commit's
      build): the same kernels and the same bits, so the same time within the spread;
  (c) with --kernel_stats DIR: device time of the wide launches alone, from the *kernel_stats.csv of
          rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python scripts/bench_rnn_wide.py --target
      (--target: five training steps and two encode calls per cell at H = 512, nothing else).  A launch walks 214 steps (the longest clip
      of the batch), a workgroup streams its direction's W_hh once per step: the implied rate is 4*G*H*H bytes / (launch time / 214).
   python scripts/bench_rnn_wide.py [--parent_lib parent/libtennis_hip.so] [--kernel_stats DIR] [--out profiles/rnn_wide_bench.json]"""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

B, T, F, E, V, L, BEAM, MAXLEN = 32, 214, 1024, 100, 254, 20, 5, 150          # config C5
LR = 1e-3
GATES = {"gru": 3, "lstm": 4}


def summary(ts, digits=4):
    return {"median": round(float(np.median(ts)), digits), "min": round(min(ts), digits), "max": round(max(ts), digits),
            "spread": round(max(ts) - min(ts), digits), "runs": [round(t, digits) for t in ts]}


def device_ms(fn, n):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0.record()
    for _ in range(n):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / n


def inputs(cell, H):
    from tennis_amd import weights as W
    p = W.make_gnmt_weights(9, cell, F, H, E, V)
    p["gnmt_tgt_proj_weight"] = (p["gnmt_tgt_proj_weight"] * 30.0).astype(np.float32)
    rng = np.random.default_rng(3)
    src = (np.abs(rng.normal(0, 1, (B, T, F))) * 0.5).astype(np.float32)
    svl = rng.integers(T // 4, T + 1, B).astype(np.int32)
    svl[0] = T                                                 # the longest clip sets every recurrent launch's step count
    tgt = rng.integers(4, V, (B, L)).astype(np.int32)
    tgt[:, 0], tgt[:, -1] = 2, 3
    dev = lambda a: torch.from_numpy(a).cuda()
    return p, dev(src), dev(svl), dev(tgt), dev(np.full(B, L, np.int32))


def routes(cells, widths):
    """{(cell, H): (training step, encode + beam search)} on handles of their own"""
    from tennis_amd.engine import GNMTCaptioner, GNMTTrainer
    out = {}
    for cell in cells:
        for H in widths:
            p, src, svl, tgt, tvl = inputs(cell, H)
            tr = GNMTTrainer(p, F, H, E, V, max_batch=B, max_src_len=T, max_tgt_len=L, cell_type=cell)
            cap = GNMTCaptioner(p, F, H, E, V, beam=BEAM, max_length=MAXLEN, max_batch=B, max_src_len=T, cell_type=cell)

            def train(tr=tr, a=(src, svl, tgt, tvl)):
                tr.forward_backward(*a)
                tr.step(LR)

            def infer(cap=cap, src=src, svl=svl):
                cap.encode(src, svl)
                cap.beam_search(2, 3, 1.0, 5.0)

            out[(cell, H)] = (train, infer)
    return out


def bench(cells, widths, steps, calls, warmup, reps):
    rs = routes(cells, widths)
    for _ in range(warmup):
        for train, infer in rs.values():
            train()
            infer()
    ms = {k: ([], []) for k in rs}
    for _ in range(reps):                                      # alternating
        for k, (train, infer) in rs.items():
            ms[k][0].append(device_ms(train, steps))
            ms[k][1].append(device_ms(infer, calls))
    return [{"cell": cell, "hidden": H, "gate_rows": GATES[cell] * H, "kernels": "wide" if GATES[cell] * H > 1024 else "one row per thread",
             "timed_steps": steps, "timed_calls": calls, "train_step_ms": summary(a), "encode_beam_search_ms": summary(b)}
            for (cell, H), (a, b) in ms.items()]


def target(cells):
    """what the kernel trace looks at: H = 512 only"""
    for (cell, H), (train, infer) in routes(cells, [512]).items():
        for _ in range(5):
            train()
        for _ in range(2):
            infer()
    torch.cuda.synchronize()


def kernel_stats(d):
    """the wide kernels' rows of rocprofv3's kernel statistics under d -> per-launch time and the implied W_hh stream rate"""
    files = sorted(glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True))
    if not files:
        return {"error": f"no *kernel_stats.csv under {d}"}
    out = []
    for row in csv.DictReader(open(files[-1])):
        name = row["Name"]
        if "wide_kernel<" not in name:
            continue
        kern = name.split("::")[-1].split("(")[0]
        g = int(kern.split("<")[1].split(",")[0])              # rnn_recurrent_wide_kernel<G, NB> / rnn_bptt_wide_kernel<G, NB>
        avg_us = float(row["AverageNs"]) / 1e3
        per_step_us = avg_us / T
        out.append({"kernel": kern, "hidden": 512, "launches": int(row["Calls"]), "average_us_per_launch": round(avg_us, 1),
                    "min_us": round(float(row["MinNs"]) / 1e3, 1), "max_us": round(float(row["MaxNs"]) / 1e3, 1), "steps_per_launch": T,
                    "us_per_step": round(per_step_us, 2), "w_hh_bytes_per_workgroup_per_step": 4 * g * 512 * 512,
                    "implied_stream_GB_per_s_per_workgroup": round(4 * g * 512 * 512 / per_step_us / 1e3, 1)})
    return {"source": "rocprofv3 --kernel-trace --stats, 5 training steps + 2 encode calls per cell at H = 512 (two encoder layers: a "
                      "bidirectional launch of 64 workgroups and a unidirectional one of 32 in every pass)", "kernels": out}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20, help="timed training steps per run")
    ap.add_argument("--calls", type=int, default=5, help="timed encode + beam-search calls per run")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--cells", default="gru,lstm")
    ap.add_argument("--widths", default="256,512")
    ap.add_argument("--parent_lib", default=None, help="libtennis_hip.so of the parent commit: the H = 256 rows are also timed on it")
    ap.add_argument("--child", action="store_true", help="(the child process of --parent_lib) print the rows only")
    ap.add_argument("--target", action="store_true", help="run the H = 512 steps once, for a kernel trace, and exit")
    ap.add_argument("--kernel_stats", default=None, help="directory of a rocprofv3 --kernel-trace --stats run of --target")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rnn_wide_bench.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_rnn_wide needs the GPU: there is nothing to time without it"
    cells, widths = a.cells.split(","), [int(w) for w in a.widths.split(",")]
    if a.target:
        target(cells)
        return
    if a.child:                                                # a library without the newer entry points: bind what it has
        import ctypes
        from tennis_amd import _lib
        have = ctypes.CDLL(_lib.LIB_PATH)
        for name in [n for n in _lib._SIGS if not hasattr(have, n)]:
            del _lib._SIGS[name]
        print(json.dumps(bench(cells, widths, a.steps, a.calls, a.warmup, a.reps)))
        return
    res = {"device": torch.cuda.get_device_name(0),
           "what": "captioner at config C5's shapes (32 x 214 x 1024, E 100, V 254, 20-token captions, beam 5, 150 decoding steps): device ms "
                   "per training step and per encode + beam search, H = 256 (one gate row per thread) and H = 512 (the wide kernels)",
           "reps": a.reps, "rows": bench(cells, widths, a.steps, a.calls, a.warmup, a.reps)}
    for r in res["rows"]:
        print(json.dumps(r), flush=True)
    if a.parent_lib:                                           # a fresh child process: one library per process
        cmd = [sys.executable, os.path.abspath(__file__), "--child", "--steps", str(a.steps), "--calls", str(a.calls), "--warmup", str(a.warmup),
               "--reps", str(a.reps), "--cells", a.cells, "--widths", "256"]
        env = dict(os.environ, TENNIS_HIP_LIB=os.path.abspath(a.parent_lib))
        out = subprocess.run(cmd, env=env, check=True, capture_output=True, text=True, timeout=300).stdout.strip().splitlines()[-1]
        res["h256_on_the_parent_build"] = json.loads(out)
        print(out, flush=True)
    else:
        res["h256_on_the_parent_build"] = "NOT MEASURED in this run (no --parent_lib)"
    res["wide_launches_alone"] = kernel_stats(a.kernel_stats) if a.kernel_stats else "NOT MEASURED in this run (no --kernel_stats)"
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
