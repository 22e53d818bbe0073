"""What returning the decoder's attention weights costs, and that not asking for them costs nothing, at config C5's shapes as
scripts/bench_rnn_wide.py sets them up (32 clips x 214 steps x 1024 features, H = 256, E = 100, V = 254, beam 5, 150 decoding steps,
20-token captions), GRU and LSTM:
  (a) encode + beam search, device ms per call, weights off (``beam_search``) and on (``beam_search(return_attention=True)``: the steps'
      rows into the history, then the ancestor-row table and the gather);
  (b) teacher forcing over 20 tokens (``decode_seq`` after one encode), device ms per call, weights off and on (one more store per step).
Same box; every run is a fresh process (one library per process), this build and - with --parent_lib - the parent commit's build
alternating, --reps runs each; medians, spread and every run are kept.  The parent's library has no "on".  The one requirement:
"off" on this build equals "off" on the parent's within the spread of the runs (``off_equals_parent``).  The cost of "on" has no bar.
With --kernel_stats DIR the "on" cost is split into the gather's two kernels (the store is inside dec_attention_kernel and has no
launch of its own), from the *kernel_stats.csv of
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python scripts/bench_gnmt_attention.py --target
  python scripts/bench_gnmt_attention.py [--parent_lib parent/libtennis_hip.so] [--kernel_stats DIR] [--out profiles/gnmt_attention_bench.json]"""
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

B, T, F, H, E, V, L, BEAM, MAXLEN = 32, 214, 1024, 256, 100, 254, 20, 5, 150          # config C5


def summary(ts, digits=4):
    return {"median": round(float(np.median(ts)), digits), "min": round(min(ts), digits), "max": round(max(ts), digits),
            "spread": round(max(ts) - min(ts), digits), "runs": [round(t, digits) for t in ts]}


def one_run(cells, calls, warmup):
    """one process' measurement: {cell: {beam_off, beam_on, tf_off, tf_on (ms per call), sample_width}}; "on" only where the library has it"""
    import ctypes
    import torch
    from tennis_amd import _lib
    have = ctypes.CDLL(_lib.LIB_PATH)
    for name in [n for n in _lib._SIGS if not hasattr(have, n)]:        # a library without the newer entry points: bind what it has
        del _lib._SIGS[name]
    has_on = hasattr(have, "tn_gnmt_beam_search_attention")
    from scripts.bench_rnn_wide import device_ms, inputs
    from tennis_amd.engine import GNMTCaptioner
    out = {}
    for cell in cells:
        p, src, svl, tgt, _ = inputs(cell, H)
        cap = GNMTCaptioner(p, F, H, E, V, beam=BEAM, max_length=MAXLEN, max_batch=B, max_src_len=T, cell_type=cell)

        def beam(on, cap=cap, src=src, svl=svl):
            cap.encode(src, svl)
            return cap.beam_search(2, 3, 1.0, 5.0, return_attention=True) if on else cap.beam_search(2, 3, 1.0, 5.0)

        def tf(on, cap=cap, tgt=tgt):
            return cap.decode_seq(tgt, return_attention=True) if on else cap.decode_seq(tgt)

        modes = (False, True) if has_on else (False,)
        for _ in range(warmup):
            for on in modes:
                beam(on)
                tf(on)
        row = {"sample_width": int(beam(False)[0].shape[2])}
        for on in modes:                                                # off and on alternate inside the run as well
            row["beam_on" if on else "beam_off"] = device_ms(lambda: beam(on), calls)
            row["tf_on" if on else "tf_off"] = device_ms(lambda: tf(on), 4 * calls)
        out[cell] = row
    return out


def target(cells):
    """what the kernel trace looks at: five encode + beam search calls with the weights on, per cell"""
    import torch
    from scripts.bench_rnn_wide import inputs
    from tennis_amd.engine import GNMTCaptioner
    for cell in cells:
        p, src, svl, _, _ = inputs(cell, H)
        cap = GNMTCaptioner(p, F, H, E, V, beam=BEAM, max_length=MAXLEN, max_batch=B, max_src_len=T, cell_type=cell)
        for _ in range(5):
            cap.encode(src, svl)
            cap.beam_search(2, 3, 1.0, 5.0, return_attention=True)
    torch.cuda.synchronize()


def kernel_stats(d):
    files = sorted(glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True))
    if not files:
        return {"error": f"no *kernel_stats.csv under {d}"}
    out = []
    for row in csv.DictReader(open(files[-1])):
        if "beam_att_" in row["Name"] or "dec_attention_kernel" in row["Name"]:
            out.append({"kernel": row["Name"].split("::")[-1].split("(")[0], "launches": int(row["Calls"]),
                        "average_us_per_launch": round(float(row["AverageNs"]) / 1e3, 2), "total_us": round(float(row["TotalDurationNs"]) / 1e3, 1)})
    return {"source": "rocprofv3 --kernel-trace --stats of --target (five searches with the weights on per cell)", "kernels": out}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=5, help="timed encode + beam-search calls per run (teacher forcing: four times as many)")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--cells", default="gru,lstm")
    ap.add_argument("--parent_lib", default=None, help="libtennis_hip.so of the parent commit: its 'off' is timed in alternation")
    ap.add_argument("--child", action="store_true", help="(a run's process) print the run's figures only")
    ap.add_argument("--target", action="store_true", help="run the searches with the weights on once, for a kernel trace, and exit")
    ap.add_argument("--kernel_stats", default=None, help="directory of a rocprofv3 --kernel-trace --stats run of --target")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gnmt_attention_bench.json"))
    a = ap.parse_args()
    cells = a.cells.split(",")
    if a.target:
        target(cells)
        return
    if a.child:
        print(json.dumps(one_run(cells, a.calls, a.warmup)))
        return
    import torch
    assert torch.cuda.is_available(), "bench_gnmt_attention needs the GPU: there is nothing to time without it"
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--calls", str(a.calls), "--warmup", str(a.warmup), "--cells", a.cells]
    builds = {"this": None, "parent": os.path.abspath(a.parent_lib) if a.parent_lib else None}
    runs = {b: [] for b in builds if b == "this" or builds[b]}
    for rep in range(a.reps):                                          # alternating, a fresh process per run
        for b in runs:
            env = dict(os.environ, TENNIS_HIP_LIB=builds[b]) if builds[b] else dict(os.environ)
            out = subprocess.run(cmd, env=env, check=True, capture_output=True, text=True, timeout=300).stdout.strip().splitlines()[-1]
            print(b, rep, out, flush=True)
            runs[b].append(json.loads(out))
    rows = []
    for cell in cells:
        row = {"cell": cell, "sample_width": runs["this"][0][cell]["sample_width"], "timed_calls": a.calls}
        for key in ("beam_off", "beam_on", "tf_off", "tf_on"):
            row[key + "_ms"] = summary([r[cell][key] for r in runs["this"]])
        for what, nm in (("beam", "encode_beam_search"), ("tf", "teacher_forcing_20_tokens")):
            off, on = row[what + "_off_ms"], row[what + "_on_ms"]
            row[nm + "_cost_of_on_ms"] = round(on["median"] - off["median"], 4)
            row[nm + "_cost_of_on_percent"] = round(100.0 * (on["median"] - off["median"]) / off["median"], 2)
            if "parent" in runs:
                par = summary([r[cell][what + "_off"] for r in runs["parent"]])
                row[what + "_off_parent_ms"] = par
                row[what + "_off_minus_parent_ms"] = round(off["median"] - par["median"], 4)          # negative: this build is faster
                row[what + "_off_equals_parent"] = bool(abs(off["median"] - par["median"]) <= max(off["spread"], par["spread"]))
                row[what + "_off_not_slower_than_parent"] = bool(off["median"] - par["median"] <= max(off["spread"], par["spread"]))
        rows.append(row)
        print(json.dumps(row), flush=True)
    att_bytes = 4 * B * BEAM * (MAXLEN + 1) * T
    res = {"device": torch.cuda.get_device_name(0),
           "what": "captioner at config C5's shapes (32 x 214 x 1024, H 256, E 100, V 254, beam 5, 150 decoding steps, 20-token captions): device "
                   "ms per encode + beam search and per teacher-forced decode_seq, attention weights off and on; every run a fresh process, "
                   "this build and the parent's alternating",
           "reps": a.reps, "history_bytes_this_handle": 4 * MAXLEN * B * BEAM * T, "attention_output_bytes": att_bytes, "rows": rows,
           "parent_build": "timed" if "parent" in runs else "NOT MEASURED in this run (no --parent_lib)",
           "store_and_gather_split": kernel_stats(a.kernel_stats) if a.kernel_stats else "NOT MEASURED in this run (no --kernel_stats)"}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
