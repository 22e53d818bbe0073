"""The fp32x3 encoder mode (TN_ENC_FP32X3, csrc/dense_fp32x3.hip) against the fp32 mode (TN_ENC_FP32, csrc/dense_fp32.hip) on the
same box: frames/s at batch 256 for 224 x 224 and 512 x 512 (pipelined forwards, as bench.py drives the default mode), the two
modes ALTERNATING, three runs each, and where the time goes in both (tn_densenet121_profile, per-family milliseconds side by side).
   python scripts/bench_fp32x3_mode.py [--sizes 224,512] [--batch 256] [--steps 10] [--out FILE.json]
(the record kept in the repository: --out profiles/fp32x3_mode_bench.json)"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from tennis_amd import weights as W  # noqa: E402
from tennis_amd.engine import DenseNet121Features  # noqa: E402

MODES = ("fp32", "fp32x3")
MFMA_CEILING = 16.0 / 6.0      # six bf16 MFMAs per k against the f32 MFMA at 1/16 of the bf16 rate: arithmetic, not a measurement


def timed(enc, x, out, steps):
    t0 = time.perf_counter()
    for _ in range(steps):
        enc(x, out=out)
    enc.join(0)
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def families(enc, x):
    stats, _ = enc.profile(x)          # (the first profiled pass warms the event pool; the second is kept)
    stats, _ = enc.profile(x)
    return {s["name"]: {"launches": s["launches"], "ms": round(s["ms"], 3),
                        "tflops": round(s["flops"] / max(s["ms"], 1e-9) / 1e9, 1) if s["flops"] else None} for s in stats}


def measure(size, batch, steps, p):
    encs = {m: DenseNet121Features(p, size, max_batch=batch, **{m: True}) for m in MODES}
    g = torch.Generator(device="cuda")
    g.manual_seed(1)
    x = torch.randint(0, 256, (batch, size, size, 3), generator=g, device="cuda", dtype=torch.uint8)
    outs = {m: torch.empty((batch, encs[m].feature_dim), dtype=torch.float32, device="cuda") for m in MODES}
    for m in MODES:
        encs[m].set_pipelined(True)
        timed(encs[m], x, outs[m], 2)
    runs = {m: [] for m in MODES}
    for _ in range(3):                  # alternating: a drift of the box's clocks lands on both modes
        for m in MODES:
            runs[m].append(batch * steps / timed(encs[m], x, outs[m], steps))
    for m in MODES:
        encs[m].set_pipelined(False)
    fams = {m: families(encs[m], x) for m in MODES}
    table = {}
    for name, f in fams["fp32"].items():
        fx = fams["fp32x3"].get(name.replace("fp32_", "fp32x3_", 1) if name.startswith("fp32_") else name)
        table[name[len("fp32_"):] if name.startswith("fp32_") else name] = {
            "launches": f["launches"], "fp32_ms": f["ms"], "fp32x3_ms": fx["ms"] if fx else None,
            "ratio": round(f["ms"] / fx["ms"], 2) if fx and fx["ms"] > 0 else None, "fp32x3_tflops": fx["tflops"] if fx else None}
    pairs = [round(b / a, 3) for a, b in zip(runs["fp32"], runs["fp32x3"])]
    spread = {m: round((max(runs[m]) - min(runs[m])) / min(runs[m]), 4) for m in MODES}
    return {"size": size, "batch": batch, "steps": steps,
            "frames_per_s": {m: [round(v, 1) for v in runs[m]] for m in MODES},
            "speedup_per_pairing": pairs, "speedup_min": min(pairs), "spread_of_own_runs": spread,
            "faster_in_every_pairing_by_more_than_the_spread": all(min(runs["fp32x3"]) > v for v in runs["fp32"]) and
            min(pairs) - 1.0 > max(spread.values()),
            "fraction_of_mfma_ceiling": round(min(pairs) / MFMA_CEILING, 3),
            "feature_max_abs_diff_between_modes": float((outs["fp32"] - outs["fp32x3"]).abs().max()),
            "workspace_gb": round(encs["fp32x3"].workspace_bytes / 1e9, 2), "families": table}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="224,512")
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--out", help="also write the JSON record to this file")
    a = ap.parse_args()
    p = W.make_densenet121_weights(0, fp16_model=False)
    res = {"modes": ["TN_ENC_FP32", "TN_ENC_FP32X3"], "mfma_ceiling": round(MFMA_CEILING, 3), "device": torch.cuda.get_device_name(0), "runs": []}
    for size in (int(s) for s in a.sizes.split(",")):
        r = measure(size, a.batch, a.steps, p)
        res["runs"].append(r)
        print(json.dumps({k: v for k, v in r.items() if k != "families"}), flush=True)
        for n, f in r["families"].items():
            print("   %-28s %3d launches  fp32 %9.3f ms  fp32x3 %9.3f ms  x %s" % (n, f["launches"], f["fp32_ms"], f["fp32x3_ms"] or 0.0, f["ratio"]),
                  flush=True)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        json.dump(res, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
