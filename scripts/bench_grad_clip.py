"""Global-norm gradient clipping (tn_<handle>_set_clip; train_gnmt --apply_clip, train --clip_grad_norm): what it costs a step, and that
a build with it switched off runs what the parent commit's build runs.  Device time per step (forward_backward + step, device
events around --steps steps) of
  * the captioner's training step at config C5's shapes (32 clips, T = 214, F = 1024, E = 100, V = 254, 20-token captions;
    scripts/time_c5.py, docs/measurement.md), GRU and LSTM at H = 256 and H = 512;
  * the fine-tuning step at 224 x 224, 64 frames;
in three states: `parent` (--parent_lib, the parent commit's libtennis_hip.so; skipped without it), `off` (this build, clipping
never switched on) and `on` (this build, set_clip with a threshold far above the norm: the reduction and the clipped update kernels
run, the scale is 1 and the parameters follow the same trajectory).  Same box; every measurement is a fresh child process (one
library per process) and the states alternate, --reps rounds.  The condition: `off` equals `parent` within the spread of the runs.
   python scripts/bench_grad_clip.py [--parent_lib build_of_parent/libtennis_hip.so] [--out profiles/grad_clip_bench.json]"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

B, T, F, E, V, L = 32, 214, 1024, 100, 254, 20          # config C5
FT_SIDE, FT_FRAMES = 224, 64
LR = 1e-3
FAR = 1e30                                              # a threshold no gradient reaches: scale = 1


def summary(ts, digits=4):
    return {"median": round(float(np.median(ts)), digits), "min": round(min(ts), digits), "max": round(max(ts), digits),
            "spread": round(max(ts) - min(ts), digits), "runs": [round(t, digits) for t in ts]}


def device_ms_per_step(step, steps):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0.record()
    for _ in range(steps):
        step()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / steps


def captioner_step(cell, hidden, clip):
    from tennis_amd import weights as W
    from tennis_amd.engine import GNMTTrainer
    p = W.make_gnmt_weights(9, cell, F, hidden, E, V)
    rng = np.random.default_rng(3)
    lens = rng.integers(T // 4, T + 1, B).astype(np.int32)
    lens[0] = T
    src = (np.abs(rng.normal(0, 1, (B, T, F))) * 0.5).astype(np.float32)
    tgt = rng.integers(4, V, (B, L)).astype(np.int32)
    tgt[:, 0], tgt[:, -1] = 2, 3
    dev = lambda a: torch.from_numpy(a).cuda()
    args = (dev(src), dev(lens), dev(tgt), dev(np.full(B, L, np.int32)))
    tr = GNMTTrainer(p, F, hidden, E, V, max_batch=B, max_src_len=T, max_tgt_len=L, cell_type=cell)
    if clip:
        tr.set_clip(FAR)

    def step():
        tr.forward_backward(*args)
        tr.step(LR)
    return tr, step


def finetune_step(clip):
    from tennis_amd import weights as W
    from tennis_amd.engine import FrameModelTrainer
    p = W.make_densenet121_weights(0)
    p.update(W.make_dense_weights(1, 11, 1024, "framemodel0_dense0_"))
    x = torch.from_numpy(W.normalize_to_nchw_f32(W.synthetic_frames_u8(FT_FRAMES, FT_SIDE, 5))).cuda().permute(0, 2, 3, 1).contiguous()
    y = torch.from_numpy(np.random.default_rng(5).integers(0, 11, FT_FRAMES).astype(np.int32)).cuda()
    tr = FrameModelTrainer(p, FT_SIDE, 11, batch=FT_FRAMES)
    if clip:
        tr.set_clip(FAR)

    def step():
        tr.forward_backward(x, y)
        tr.step(FT_FRAMES, 1e-3, 0.9, 1e-4)
    return tr, step


def shapes(only):
    out = [(f"captioner_{cell}_H{h}", lambda clip, c=cell, hh=h: captioner_step(c, hh, clip)) for cell in ("gru", "lstm") for h in (256, 512)]
    out.append((f"finetune_{FT_SIDE}x{FT_FRAMES}", finetune_step))
    return [s for s in out if not only or s[0] in only]


def child(a):
    """one state, every shape: {shape: ms per step}; with clipping on also the last step's (norm, scale, clipped steps)"""
    import ctypes
    from tennis_amd import _lib
    have = ctypes.CDLL(_lib.LIB_PATH)                       # the parent's library has no clip entry points: bind what it has
    for name in [n for n in _lib._SIGS if not hasattr(have, n)]:
        del _lib._SIGS[name]
    out = {}
    for name, make in shapes(a.shapes):
        tr, step = make(a.child == "on")
        for _ in range(a.warmup):
            step()
        out[name] = {"ms": device_ms_per_step(step, a.steps)}
        if a.child == "on":
            norm, scale, clipped = tr.clip_stats()
            out[name].update(norm=norm, scale=scale, clipped_steps=clipped)
        del tr, step
        torch.cuda.empty_cache()
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50, help="timed steps per measurement")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--shapes", nargs="*", default=None, help="a subset of the shapes by name (default: all)")
    ap.add_argument("--parent_lib", default=None, help="libtennis_hip.so of the parent commit")
    ap.add_argument("--child", default=None, choices=["parent", "off", "on"], help="(internal) measure one state and print it")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "grad_clip_bench.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_grad_clip needs the GPU: there is nothing to time without it"
    if a.child:
        return child(a)
    states = (["parent"] if a.parent_lib else []) + ["off", "on"]
    runs = {s: [] for s in states}
    for _ in range(a.reps):                                 # alternating; one process, one library, at a time
        for s in states:
            cmd = [sys.executable, os.path.abspath(__file__), "--child", s, "--steps", str(a.steps), "--warmup", str(a.warmup)]
            if a.shapes:
                cmd += ["--shapes"] + a.shapes
            env = dict(os.environ)
            if s == "parent":
                env["TENNIS_HIP_LIB"] = os.path.abspath(a.parent_lib)
            else:
                env.pop("TENNIS_HIP_LIB", None)
            line = subprocess.run(cmd, env=env, check=True, capture_output=True, text=True, timeout=600).stdout.strip().splitlines()[-1]
            runs[s].append(json.loads(line))
            print(s, line, flush=True)
    res = {"device": torch.cuda.get_device_name(0),
           "what": "device ms per training step (forward_backward + step): the parent commit's build, this build with clipping off, this "
                   "build with clipping on (threshold never reached: the reduction and the clipped update kernels run, scale 1)",
           "reps": a.reps, "timed_steps": a.steps, "shapes": []}
    if not a.parent_lib:
        res["parent"] = "NOT MEASURED in this run (no --parent_lib)"
    for name, _ in shapes(a.shapes):
        row = {"shape": name}
        for s in states:
            row[f"{s}_ms_per_step"] = summary([r[name]["ms"] for r in runs[s]])
        off, on = row["off_ms_per_step"], row["on_ms_per_step"]
        row["on_minus_off_ms"] = round(on["median"] - off["median"], 4)
        row["on_minus_off_percent_of_step"] = round(100 * (on["median"] - off["median"]) / off["median"], 3)
        if a.parent_lib:
            par = row["parent_ms_per_step"]
            row["off_minus_parent_ms"] = round(off["median"] - par["median"], 4)
            row["off_equals_parent_within_spread"] = bool(abs(off["median"] - par["median"]) <= max(off["spread"], par["spread"]))
        last = runs["on"][-1][name]
        row["on_last_step"] = {"norm": last["norm"], "scale": last["scale"], "clipped_steps": last["clipped_steps"]}
        res["shapes"].append(row)
        print(json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
