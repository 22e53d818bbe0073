"""The fp32 encoder mode (TN_ENC_FP32, csrc/dense_fp32.hip): frames/s at batch 256 for 224 x 224 and 512 x 512 (pipelined forwards,
as bench.py drives the default mode) and where the time goes (tn_densenet121_profile), each family's share of the 157.3 TF f32
matrix peak.   python scripts/bench_fp32_mode.py [--sizes 224,512] [--batch 256] [--steps 10] [--out FILE.json]
(the record kept in the repository: --out profiles/fp32_mode_bench.json)"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from tennis_amd import weights as W  # noqa: E402
from tennis_amd.engine import DenseNet121Features  # noqa: E402

F32_PEAK_TF = 157.3      # v_mfma_f32_32x32x2_f32 / 16x16x4_f32: 64 FLOP/clk/SIMD


def measure(size, batch, steps, p):
    enc = DenseNet121Features(p, size, max_batch=batch, fp32=True)
    g = torch.Generator(device="cuda")
    g.manual_seed(1)
    x = torch.randint(0, 256, (batch, size, size, 3), generator=g, device="cuda", dtype=torch.uint8)
    out = torch.empty((batch, enc.feature_dim), dtype=torch.float32, device="cuda")
    enc.set_pipelined(True)
    for _ in range(2):
        enc(x, out=out)
    enc.join(0)
    torch.cuda.synchronize()
    ts = []
    for _ in range(3):
        t0 = time.perf_counter()
        for _ in range(steps):
            enc(x, out=out)
        enc.join(0)
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    enc.set_pipelined(False)
    dt = float(np.median(ts))
    fps = batch * steps / dt
    stats, _ = enc.profile(x)          # (the first profiled pass warms the event pool; the second is kept)
    stats, _ = enc.profile(x)
    flops = sum(s["flops"] for s in stats)
    total_ms = sum(s["ms"] for s in stats)
    fams = {s["name"]: {"launches": s["launches"], "ms": round(s["ms"], 3), "share": round(s["ms"] / total_ms, 4),
                        "tflops": round(s["flops"] / max(s["ms"], 1e-9) / 1e9, 1) if s["flops"] else None,
                        "frac_of_f32_peak": round(s["flops"] / max(s["ms"], 1e-9) / 1e9 / F32_PEAK_TF, 3) if s["flops"] else None}
            for s in stats}
    return {"size": size, "batch": batch, "steps": steps, "frames_per_s": round(fps, 1), "ms_per_batch": round(dt / steps * 1e3, 2),
            "tflop_per_batch": round(flops / 1e12, 3), "tflops": round(fps / batch * flops / 1e12, 1),
            "frac_of_f32_peak": round(fps / batch * flops / 1e12 / F32_PEAK_TF, 3),
            "workspace_gb": round(enc.workspace_bytes / 1e9, 2), "profile_ms_unsplit": round(total_ms, 2), "families": fams}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="224,512")
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--out", help="also write the JSON record to this file")
    a = ap.parse_args()
    p = W.make_densenet121_weights(0, fp16_model=False)
    res = {"mode": "TN_ENC_FP32", "f32_peak_tflops": F32_PEAK_TF, "device": torch.cuda.get_device_name(0), "runs": []}
    for size in (int(s) for s in a.sizes.split(",")):
        r = measure(size, a.batch, a.steps, p)
        res["runs"].append(r)
        print(json.dumps({k: v for k, v in r.items() if k != "families"}), flush=True)
        for n, f in r["families"].items():
            print("   %-28s %3d launches %9.3f ms  %5.1f %%  %s TF  %s of peak" % (n, f["launches"], f["ms"], 100 * f["share"], f["tflops"],
                                                                              f["frac_of_f32_peak"]), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        json.dump(res, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
