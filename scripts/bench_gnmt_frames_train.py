"""The frame-mode captioner training step (engine.GNMTFramesTrainer, tn_gnmt_frames_trainer_*): ms per step at 224 x 224 with 4 clips x
16 frames (64 frames), GRU, hidden 128, target length 20, trainable and frozen backbone - next to its two parts measured in the same
run: the backbone-only step on the same 64 frames (engine.FrameModelTrainer) and the feature-mode captioner step on the same shapes
(engine.GNMTTrainer on (4, 16, 1024) features).  The frame-mode step is to be judged against the sum of the two.  Each figure is the
median of --reps timed runs of --steps (forward_backward + step) after --warmup; the runs are kept, so the spread is on record.
   python scripts/bench_gnmt_frames_train.py [--size 224] [--batch 4] [--steps_src 16] [--tgt_len 20] [--steps 10] [--out FILE.json]
(the record kept in the repository: --out profiles/gnmt_frames_train_bench.json)"""
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
from tennis_amd.engine import FrameModelTrainer, GNMTFramesTrainer, GNMTTrainer  # noqa: E402


def timed(fb, step, steps, warmup, reps):
    for _ in range(warmup):
        fb()
        step()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        for _ in range(steps):
            fb()
            step()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) / steps * 1e3)
    return {"ms_per_step": round(float(np.median(ts)), 2), "ms_per_step_runs": [round(t, 2) for t in ts],
            "spread_ms": round(float(max(ts) - min(ts)), 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=224)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--steps_src", type=int, default=16)
    ap.add_argument("--tgt_len", type=int, default=20)
    ap.add_argument("--hidden", type=int, default=128)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", help="also write the JSON record to this file")
    a = ap.parse_args()
    B, T, S, L, H, n = a.batch, a.steps_src, a.size, a.tgt_len, a.hidden, a.batch * a.steps_src
    E, V = 100, 254
    p = W.make_densenet121_weights(0)
    p.update(W.make_gnmt_weights(3, "gru", 1024, H, E, V))
    p.update(W.make_dense_weights(1, 11, 1024, "framemodel0_dense0_"))
    g = torch.Generator(device="cuda")
    g.manual_seed(1)
    x = torch.randn((n, S, S, 3), generator=g, device="cuda")
    feats = torch.rand((B, T, 1024), generator=g, device="cuda")
    y_frame = torch.randint(0, 11, (n,), generator=g, device="cuda", dtype=torch.int32)
    svl = torch.full((B,), T, dtype=torch.int32, device="cuda")
    svl[1:] -= torch.arange(1, B, dtype=torch.int32, device="cuda")          # clips of different lengths: padded slots in the batch
    tgt = torch.randint(4, V, (B, L), generator=g, device="cuda", dtype=torch.int32)
    tgt[:, 0], tgt[:, -1] = 2, 3
    tvl = torch.full((B,), L, dtype=torch.int32, device="cuda")
    res = {"device": torch.cuda.get_device_name(0), "size": S, "batch": B, "src_steps": T, "frames_per_step": n, "cell": "gru", "hidden": H,
           "tgt_len": L, "steps": a.steps, "warmup": a.warmup, "reps": a.reps, "runs": {}}

    def record(name, fb, step):
        res["runs"][name] = timed(fb, step, a.steps, a.warmup, a.reps)
        torch.cuda.synchronize()
        print(name, json.dumps(res["runs"][name]), flush=True)

    clips = x.view(B, T, S, S, 3)
    for name, frozen in (("frames_trainable", False), ("frames_frozen", True)):
        tr = GNMTFramesTrainer(p, H, E, V, size=S, max_batch=B, max_src_len=T, max_tgt_len=L, freeze_backbone=frozen)
        record(name, lambda: tr.forward_backward(clips, svl, tgt, tvl), lambda: tr.step(1e-4))
        del tr
    fm = FrameModelTrainer(p, S, 11, batch=n)
    record("framemodel_%d" % n, lambda: fm.forward_backward(x, y_frame), lambda: fm.step(n, 1e-4, 0.9, 1e-4))
    del fm
    cap = GNMTTrainer(p, 1024, H, E, V, max_batch=B, max_src_len=T, max_tgt_len=L)
    record("captioner_features", lambda: cap.forward_backward(feats, svl, tgt, tvl), lambda: cap.step(1e-4))
    del cap
    parts = res["runs"]["framemodel_%d" % n]["ms_per_step"] + res["runs"]["captioner_features"]["ms_per_step"]
    res["sum_of_parts_ms"] = round(parts, 2)
    res["trainable_minus_parts_ms"] = round(res["runs"]["frames_trainable"]["ms_per_step"] - parts, 2)
    res["trainable_over_parts"] = round(res["runs"]["frames_trainable"]["ms_per_step"] / parts, 3)
    print(json.dumps({k: v for k, v in res.items() if k != "runs"}), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        json.dump(res, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
