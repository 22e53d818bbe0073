"""The temporal head trained from a device-resident feature table (engine.TemporalHeadTrainer.forward_backward_rows, tn_head_*_rows;
train --dense_windows) against the route it replaces.  Same box, the two routes alternating, --reps runs each; medians and every run
are kept.
  * device time per step (forward_backward + step, device events around --steps steps): the materialised step on a device-resident
    (B, T, F) batch against the gathered step on the table the batch was taken from, at 32 x 64 x 1024 and 32 x 30 x 4096, H = 128,
    GRU and LSTM.  This prices the gathered loaders alone: the batch of the materialised step is already on the device.
  * wall time per epoch: the loader route of train.py (TennisSet.__getitem__ opening one .npy per window step, the loader stacking
    (B, T, F), one host-to-device copy per batch) against the --dense_windows route (window_table + load_feature_table once, then
    device slices), over a synthetic on-disk feature set of --frames frames at window 30, batch 32; the table load is reported apart.
    The feature files are written by this script just before they are read, so the page cache is WARM for both routes.
   python scripts/bench_head_rows_train.py [--out profiles/head_rows_train_bench.json]"""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from tennis_amd import weights as W  # noqa: E402
from tennis_amd.dataset import DataLoader, TennisSet  # noqa: E402
from tennis_amd.engine import TemporalHeadTrainer  # noqa: E402
from tennis_amd.train import DeviceWindows  # noqa: E402

CLASSES, HIDDEN = 11, 128
LR, MOM, WD = 1e-3, 0.9, 1e-4


def head_params(cell, feat):
    p = W.make_rnn_weights(2, cell, feat, HIDDEN, f"cnnrnn0_{cell}0_")
    p.update(W.make_dense_weights(1, CLASSES, 2 * HIDDEN, "cnnrnn0_dense0_"))
    return p


def summary(ts, digits=4):
    return {"median": round(float(np.median(ts)), digits), "min": round(min(ts), digits), "max": round(max(ts), digits),
            "runs": [round(t, digits) for t in ts]}


def device_ms_per_step(step, batch, steps):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0.record()
    for _ in range(steps):
        step()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / steps


def bench_step(cell, B, T, F, rows, steps, warmup, reps):
    """windows as the dataset makes them: T consecutive table rows around a random centre, clamped at the table's ends"""
    p = head_params(cell, F)
    g = torch.Generator(device="cuda")
    g.manual_seed(3)
    table = torch.rand((rows, F), generator=g, device="cuda")
    centre = torch.randint(0, rows, (B, 1), generator=g, device="cuda")
    idx = (centre + torch.arange(T, device="cuda")[None, :] - T // 2).clamp_(0, rows - 1).to(torch.int32)
    y = torch.randint(0, CLASSES, (B,), generator=g, device="cuda", dtype=torch.int32)
    x = table[idx.long()].contiguous()
    mat, gat = (TemporalHeadTrainer(p, F, HIDDEN, CLASSES, max_batch=B, max_steps=T, type=cell) for _ in range(2))
    gat.set_features(table)

    def step_mat():
        mat.forward_backward(x, y)
        mat.step(B, LR, MOM, WD)

    def step_gat():
        gat.forward_backward_rows(idx, y)
        gat.step(B, LR, MOM, WD)

    for _ in range(warmup):
        step_mat()
        step_gat()
    ms = {"materialised": [], "gathered": []}
    for _ in range(reps):                                  # alternating
        ms["materialised"].append(device_ms_per_step(step_mat, B, steps))
        ms["gathered"].append(device_ms_per_step(step_gat, B, steps))
    same = bool(torch.equal(mat.params, gat.params))       # both handles took the same steps: the parameters must be the same bits
    out = {"cell": cell, "batch": B, "steps": T, "feat": F, "hidden": HIDDEN, "table_rows": rows, "timed_steps": steps,
           "materialised_ms_per_step": summary(ms["materialised"]), "gathered_ms_per_step": summary(ms["gathered"]),
           "parameters_bit_identical_after_all_steps": same}
    out["gathered_over_materialised"] = round(out["gathered_ms_per_step"]["median"] / out["materialised_ms_per_step"]["median"], 4)
    return out


def write_features(root, videos, frames, feat):
    ds = TennisSet(root=root, videos=videos, frames_per_video=frames, window=1, feats_model="0001", synthetic=True)
    rng = np.random.default_rng(0)
    for v, f, _ in ds._samples:
        path = ds.get_feature_path(ds.feat_dir, v, f)
        os.makedirs(os.path.dirname(path), exist_ok=True)
        np.save(path, rng.random(feat, dtype=np.float32))


def bench_epoch(cell, frames, feat, window, batch, reps, workdir):
    videos = ("V006", "V007")
    write_features(workdir, videos, frames // 2, feat)
    ds = TennisSet(root=workdir, videos=videos, frames_per_video=frames // 2, window=window, feats_model="0001", synthetic=True)
    dev = torch.device("cuda", torch.cuda.current_device())
    p = head_params(cell, feat)
    mk = lambda: TemporalHeadTrainer(p, feat, HIDDEN, CLASSES, max_batch=batch, max_steps=window, type=cell)
    loader_head, dense_head = mk(), mk()
    loaders = [DataLoader(ds, batch, shuffle=True, last_batch="keep") for _ in range(2)]     # same seed: the same order
    t0 = time.perf_counter()
    win = DeviceWindows(ds, feat, dev, "train", log=lambda *a: None)
    torch.cuda.synchronize()
    table_load_s = time.perf_counter() - t0
    dense_head.set_features(win.table)

    def epoch_loader():
        t0 = time.perf_counter()
        for data, labels, _ in loaders[0]:                 # what train.py's batches() does per step
            x = torch.from_numpy(np.ascontiguousarray(data)).to(dev)
            y = torch.from_numpy(labels.astype(np.int32)).to(dev)
            loader_head.forward_backward(x, y)
            loader_head.step(batch, LR, MOM, WD)
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    def epoch_dense():
        t0 = time.perf_counter()
        for rows, y in win.epoch_batches(loaders[1], lambda ids: ids):
            dense_head.forward_backward_rows(rows, y)
            dense_head.step(batch, LR, MOM, WD)
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    s = {"loader": [], "dense_windows": []}
    for _ in range(reps):                                  # alternating; no warm-up epoch: the first runs are in the spread
        s["loader"].append(epoch_loader())
        s["dense_windows"].append(epoch_dense())
    same = bool(torch.equal(loader_head.params, dense_head.params))
    out = {"cell": cell, "frames": len(ds), "feat": feat, "window": window, "batch": batch, "steps_per_epoch": len(loaders[0]),
           "page_cache": "warm (the files were written by this run just before they were read)",
           "table_rows": int(win.table.shape[0]), "table_bytes": int(win.table.numel() * 4),
           "table_load_seconds_once": round(table_load_s, 4),
           "loader_epoch_seconds": summary(s["loader"]), "dense_windows_epoch_seconds": summary(s["dense_windows"]),
           "parameters_bit_identical_after_all_epochs": same}
    out["loader_over_dense_windows"] = round(out["loader_epoch_seconds"]["median"] / out["dense_windows_epoch_seconds"]["median"], 2)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200, help="timed steps per run of the device-time part")
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--table_rows", type=int, default=20000)
    ap.add_argument("--frames", type=int, default=4096, help="frames of the on-disk feature set of the epoch part")
    ap.add_argument("--epoch_feat", type=int, default=1024)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "head_rows_train_bench.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_head_rows_train needs the GPU: there is nothing to time without it"
    res = {"device": torch.cuda.get_device_name(0),
           "what": "temporal head: gathered step (forward_backward_rows) vs materialised step, device ms per step; "
                   "loader route vs --dense_windows, wall seconds per epoch",
           "reps": a.reps, "step": [], "epoch": []}
    for cell in ("gru", "lstm"):
        for B, T, F in ((32, 64, 1024), (32, 30, 4096)):
            r = bench_step(cell, B, T, F, a.table_rows, a.steps, a.warmup, a.reps)
            res["step"].append(r)
            print(json.dumps(r), flush=True)
    for cell in ("gru", "lstm"):
        with tempfile.TemporaryDirectory() as tmp:
            r = bench_epoch(cell, a.frames, a.epoch_feat, 30, 32, a.reps, tmp)
        res["epoch"].append(r)
        print(json.dumps(r), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
