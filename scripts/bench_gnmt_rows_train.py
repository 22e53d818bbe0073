"""The captioner trained from a device-resident feature table (engine.GNMTTrainer.forward_backward_rows,
tn_gnmt_trainer_forward_backward_rows; train_gnmt --feats_on_device) against the route it replaces.  Same box, the routes alternating,
--reps runs each; medians and every run are kept.
  (a) wall time per epoch: the loader route of train_gnmt.train (CaptionSet.__getitem__ opening one .npy per frame of every point,
      pad_batchify stacking a zero-padded (B, T, F) array, one host-to-device copy per batch) against the flag's route (clip_table +
      load_clip_table + one upload, then bucketed_batches(rows=...) and the gathered step), over a synthetic on-disk tree of --points
      ragged points, F = 1024, batch 32, H = 256; the table load is reported apart.  The feature files are written by this script just
      before they are read, so the page cache is WARM for both routes.
  (b) device time per step (forward_backward + Adam step, device events around --steps steps) at config C5's shapes (32 clips, T = 214,
      F = 1024, H = 256, E = 100, V = 254, 20-token captions; scripts/time_c5.py, docs/measurement.md), ragged clip lengths:
        resident        forward_backward on a (B, T, F) batch already on the device - existing code.  With --parent_lib PATH the same
                        route is ALSO timed in a child process on that library (the parent commit's build), as the baseline;
        gathered        forward_backward_rows on the table the batch was taken from;
        gathered_noskip the same with the pad-tile skip of the gathered i2h product compiled out (tn_dbg_rows_pad_skip(0)).
   python scripts/bench_gnmt_rows_train.py [--parent_lib build_of_parent/libtennis_hip.so] [--out profiles/gnmt_rows_train_bench.json]"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

B, T, F, H, E, V, L = 32, 214, 1024, 256, 100, 254, 20          # config C5
LR = 1e-3


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


def c5_inputs(cell, rows):
    """clips as the dataset makes them: consecutive table rows from a random start; lengths ragged between T / 4 and T, one of them T"""
    from tennis_amd import weights as W
    p = W.make_gnmt_weights(9, cell, F, H, E, V)
    rng = np.random.default_rng(3)
    lens = rng.integers(T // 4, T + 1, B).astype(np.int32)
    lens[0] = T
    idx = np.full((B, T), -1, np.int32)
    for b in range(B):
        start = int(rng.integers(0, rows - T))
        idx[b, :lens[b]] = np.arange(start, start + lens[b])
    tgt = rng.integers(4, V, (B, L)).astype(np.int32)
    tgt[:, 0], tgt[:, -1] = 2, 3
    table = (np.abs(rng.normal(0, 1, (rows, F))) * 0.5).astype(np.float32)
    return p, table, idx, lens, tgt, np.full(B, L, np.int32)


def bench_step(cell, rows, steps, warmup, reps, resident_only=False):
    from tennis_amd import _lib
    from tennis_amd.engine import GNMTTrainer
    p, table, idx, lens, tgt, tvl = c5_inputs(cell, rows)
    dev = lambda a: torch.from_numpy(a).cuda()
    td, idx_d, svl, tgt_d, tvl_d = dev(table), dev(idx), dev(lens), dev(tgt), dev(tvl)
    src = torch.where((idx_d >= 0)[..., None], td[idx_d.clamp(min=0).long()], torch.zeros((), device="cuda")).contiguous()
    mk = lambda: GNMTTrainer(p, F, H, E, V, max_batch=B, max_src_len=T, max_tgt_len=L, cell_type=cell)
    routes = {"resident": mk()}
    if not resident_only:
        routes.update(gathered=mk(), gathered_noskip=mk())
    lib = _lib.load()

    def step(name):
        tr = routes[name]
        if name == "resident":
            tr.forward_backward(src, svl, tgt_d, tvl_d)
        else:
            lib.tn_dbg_rows_pad_skip(0 if name == "gathered_noskip" else 1)
            tr.forward_backward_rows(td, idx_d, svl, tgt_d, tvl_d)
        tr.step(LR)

    for _ in range(warmup):
        for name in routes:
            step(name)
    ms = {name: [] for name in routes}
    for _ in range(reps):                                  # alternating
        for name in routes:
            ms[name].append(device_ms_per_step(lambda: step(name), steps))
    if not resident_only:
        lib.tn_dbg_rows_pad_skip(1)
    pad = float((idx < 0).mean())
    tiles = [bool((idx.reshape(-1)[m:m + 64] < 0).all()) for m in range(0, B * T, 64)]
    out = {"cell": cell, "batch": B, "steps": T, "feat": F, "hidden": H, "embed": E, "vocab": V, "target_len": L, "table_rows": rows,
           "timed_steps": steps, "pad_fraction_of_rows": round(pad, 4), "all_pad_64_row_tiles": f"{sum(tiles)} of {len(tiles)}",
           **{f"{name}_ms_per_step": summary(v) for name, v in ms.items()}}
    if not resident_only:
        # every handle took the same steps: the parameters must be the same bits
        out["parameters_bit_identical_after_all_steps"] = all(bool(torch.equal(routes["resident"].params, routes[n].params))
                                                               for n in ("gathered", "gathered_noskip"))
        out["gathered_over_resident"] = round(out["gathered_ms_per_step"]["median"] / out["resident_ms_per_step"]["median"], 4)
        out["skip_minus_noskip_ms"] = round(out["gathered_ms_per_step"]["median"] - out["gathered_noskip_ms_per_step"]["median"], 4)
    return out


def write_tree(root, points, feat, mean_frames, seed=0):
    """the reference's data/ layout in feature mode: one video per split, ragged consecutive points, one .npy per frame"""
    from tennis_amd.captions import WORDS
    from tennis_amd.dataset import TennisSet
    rng = np.random.default_rng(seed)
    os.makedirs(os.path.join(root, "splits", "02"), exist_ok=True)
    os.makedirs(os.path.join(root, "annotations", "labels"), exist_ok=True)
    pts, caps, n_files = [], [], 0
    for vi, (split, n_points) in enumerate((("train", points),)):
        v, frame = f"V{100 + vi}", 0
        for i in range(n_points):
            n = int(np.clip(rng.normal(mean_frames, mean_frames / 3), 8, T))
            pts.append(f"P{split}{i:05d} {v} {frame} {frame + n}")
            caps.append(f"P{split}{i:05d}\t" + " ".join(rng.choice(WORDS, size=int(rng.integers(4, 18)))))
            frame += n
        with open(os.path.join(root, "annotations", "labels", v + ".txt"), "w") as f:
            f.write("".join(f"{fr} OTH\n" for fr in range(frame)))
        with open(os.path.join(root, "splits", "02", split + ".txt"), "w") as f:
            f.write("".join(f"{v} {fr}\n" for fr in range(frame)))
        for fr in range(frame):
            img = TennisSet.get_image_path(os.path.join(root, "frames"), v, fr)
            os.makedirs(os.path.dirname(img), exist_ok=True)
            open(img, "wb").close()                        # the dataset asks only whether the frame exists
            path = TennisSet.get_feature_path(os.path.join(root, "features", "0001"), v, fr)
            os.makedirs(os.path.dirname(path), exist_ok=True)
            np.save(path, rng.random(feat, dtype=np.float32))
        n_files += frame
    with open(os.path.join(root, "annotations", "points.txt"), "w") as f:
        f.write("\n".join(pts) + "\n")
    with open(os.path.join(root, "annotations", "captions.txt"), "w") as f:
        f.write("\n".join(caps) + "\n")
    return n_files


def bench_epoch(cell, points, feat, mean_frames, reps, workdir):
    from tennis_amd import weights as W
    from tennis_amd.captions import CaptionSet, bucketed_batches, to_device, upload_clip_table
    from tennis_amd.engine import GNMTTrainer
    n_files = write_tree(workdir, points, feat, mean_frames)
    ds = CaptionSet(split="train", root=workdir, feats_model="0001", max_cap_len=50)
    vocab = len(ds.vocab)
    p = W.make_gnmt_weights(9, cell, feat, H, E, vocab)
    max_t, max_l = max(ds.get_clip_lens()), max(l[-1] for l in ds.get_data_lens())
    mk = lambda: GNMTTrainer(p, feat, H, E, vocab, max_batch=B, max_src_len=max_t, max_tgt_len=max_l, cell_type=cell)
    loader_tr, table_tr = mk(), mk()
    t0 = time.perf_counter()
    table, rows = upload_clip_table(ds)
    torch.cuda.synchronize()
    table_load_s = time.perf_counter() - t0
    dev32 = lambda a: torch.from_numpy(a.astype(np.int32)).cuda()
    epochs = {"loader": 0, "feats_on_device": 0}

    def epoch_loader():                                    # train_gnmt.train's inner loop, loader route
        t0 = time.perf_counter()
        for src, tgt, svl, tvl in bucketed_batches(ds, B, 5, shuffle=True, seed=0, epoch=epochs["loader"]):
            loader_tr.forward_backward(to_device(src), dev32(svl), torch.from_numpy(tgt).cuda(), dev32(tvl))
            loader_tr.step(LR)
        torch.cuda.synchronize()
        epochs["loader"] += 1
        return time.perf_counter() - t0

    def epoch_table():                                     # ... and with feats_on_device
        t0 = time.perf_counter()
        for ridx, tgt, svl, tvl in bucketed_batches(ds, B, 5, shuffle=True, seed=0, epoch=epochs["feats_on_device"], rows=rows):
            table_tr.forward_backward_rows(table, ridx, svl.astype(np.int32), torch.from_numpy(tgt).cuda(), dev32(tvl))
            table_tr.step(LR)
        torch.cuda.synchronize()
        epochs["feats_on_device"] += 1
        return time.perf_counter() - t0

    s = {"loader": [], "feats_on_device": []}
    for _ in range(reps):                                  # alternating; no warm-up epoch: the first runs are in the spread
        s["loader"].append(epoch_loader())
        s["feats_on_device"].append(epoch_table())
    steps = len(list(bucketed_batches(ds, B, 5, rows=rows)))
    out = {"cell": cell, "points": len(ds), "feature_files": n_files, "frames_read_per_epoch_by_the_loader": int(sum(ds.get_clip_lens())),
           "feat": feat, "hidden": H, "batch": B, "steps_per_epoch": steps,
           "page_cache": "warm (the files were written by this run just before they were read)",
           "table_rows": int(table.shape[0]), "table_bytes": int(table.numel() * 4), "table_load_seconds_once": round(table_load_s, 4),
           "loader_epoch_seconds": summary(s["loader"]), "feats_on_device_epoch_seconds": summary(s["feats_on_device"]),
           "parameters_bit_identical_after_all_epochs": bool(torch.equal(loader_tr.params, table_tr.params))}
    out["loader_over_feats_on_device"] = round(out["loader_epoch_seconds"]["median"] / out["feats_on_device_epoch_seconds"]["median"], 2)
    out["loader_host_seconds_per_step"] = round((out["loader_epoch_seconds"]["median"] - out["feats_on_device_epoch_seconds"]["median"]) / steps, 5)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=100, help="timed steps per run of the device-time part")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--table_rows", type=int, default=20000)
    ap.add_argument("--points", type=int, default=256, help="points of the on-disk train split of the epoch part")
    ap.add_argument("--mean_frames", type=int, default=60)
    ap.add_argument("--cells", default="gru,lstm")
    ap.add_argument("--parent_lib", default=None, help="libtennis_hip.so of the parent commit: the resident route is also timed on it")
    ap.add_argument("--resident_only", action="store_true", help="(the child process of --parent_lib) print the resident route's rows only")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gnmt_rows_train_bench.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_gnmt_rows_train needs the GPU: there is nothing to time without it"
    cells = a.cells.split(",")
    if a.resident_only:                                    # a library without the rows entry points: bind what it has
        import ctypes
        from tennis_amd import _lib
        have = ctypes.CDLL(_lib.LIB_PATH)
        for name in [n for n in _lib._SIGS if not hasattr(have, n)]:
            del _lib._SIGS[name]
        print(json.dumps([bench_step(c, a.table_rows, a.steps, a.warmup, a.reps, resident_only=True) for c in cells]))
        return
    res = {"device": torch.cuda.get_device_name(0),
           "what": "captioner: gathered step (forward_backward_rows) vs the step on a resident batch, with and without the pad-tile skip, "
                   "device ms per step at config C5's shapes; loader route vs --feats_on_device, wall seconds per epoch",
           "reps": a.reps, "step": [], "epoch": []}
    for cell in cells:
        r = bench_step(cell, a.table_rows, a.steps, a.warmup, a.reps)
        res["step"].append(r)
        print(json.dumps(r), flush=True)
    if a.parent_lib:                                       # a fresh child process: one library per process
        cmd = [sys.executable, os.path.abspath(__file__), "--resident_only", "--steps", str(a.steps), "--warmup", str(a.warmup), "--reps",
               str(a.reps), "--table_rows", str(a.table_rows), "--cells", a.cells]
        env = dict(os.environ, TENNIS_HIP_LIB=os.path.abspath(a.parent_lib))
        out = subprocess.run(cmd, env=env, check=True, capture_output=True, text=True, timeout=300).stdout.strip().splitlines()[-1]
        for r, base in zip(res["step"], json.loads(out)):
            r["resident_on_the_parent_build_ms_per_step"] = base["resident_ms_per_step"]
            r["gathered_over_resident_on_the_parent_build"] = round(r["gathered_ms_per_step"]["median"] / base["resident_ms_per_step"]["median"], 4)
        print(out, flush=True)
    else:
        res["resident_on_the_parent_build"] = "NOT MEASURED in this run (no --parent_lib)"
    for cell in cells:
        with tempfile.TemporaryDirectory() as tmp:
            r = bench_epoch(cell, a.points, F, a.mean_frames, a.reps, tmp)
        res["epoch"].append(r)
        print(json.dumps(r), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
