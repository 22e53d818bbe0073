#!/usr/bin/env python3
"""Record tests/golden/encoder_routes.json: the kernel families the fp16 DenseNet-121 encoder launches, per input size, batch, TN_*
environment and create flags, as DenseNet121Features.profile() reports them on the GPU (name, launches, flops, bytes in first-seen
order; the event times are dropped).  The fixture is what tests/test_cpu_encoder_routes.py holds the device-free plan
(tn_dbg_encoder_plan) to and what tests/test_gpu_encoder_routes.py holds the launches to; re-record it only with a change that
means to move a route.

    python scripts/record_encoder_routes.py [--out tests/golden/encoder_routes.json]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SWITCHES = ("TN_NO_FUSE", "TN_NO_CHAIN", "TN_NO_BLOCK7", "TN_NO_BLOCK14", "TN_BLOCK28", "TN_NO_STRIP", "TN_NO_STRIP_CHAIN",
            "TN_DL_VARIANT", "TN_STRIP_MIN_BATCH")
EXACT = 1      # _lib.ENC_EXACT_WEIGHTS


def cases():
    """(size, batch, env, flags) of every fixture entry"""
    out = []
    for env in ({}, {"TN_STRIP_MIN_BATCH": "1"}):
        out += [(size, 2, env, 0) for size in (224, 232, 448, 512)]
    out += [(224, b, {}, 0) for b in (63, 64)]               # the strip threshold of 64 frames
    out += [(512, b, {}, 0) for b in (12, 13, 21, 22)]       # ... reached with 5 / 3 workgroups per 128 x 128 / 64 x 64 frame
    one = [{"TN_NO_FUSE": "1"}, {"TN_NO_CHAIN": "1"}, {"TN_NO_BLOCK7": "1"}, {"TN_NO_BLOCK14": "1"},
           {"TN_NO_BLOCK7": "1", "TN_NO_BLOCK14": "1"}, {"TN_NO_BLOCK7": "1", "TN_NO_BLOCK14": "1", "TN_NO_CHAIN": "1"},
           {"TN_BLOCK28": "1"}, {"TN_NO_STRIP": "1"}, {"TN_NO_STRIP_CHAIN": "1"}, {"TN_DL_VARIANT": "256"}]
    for size in (224, 448):
        out += [(size, 2, dict(env, TN_STRIP_MIN_BATCH="1"), 0) for env in one]
    out += [(224, 2, {}, EXACT), (224, 2, {"TN_DL_VARIANT": "256"}, EXACT)]
    return out


def set_env(env):
    """the encoder reads its switches when it is created"""
    for k in SWITCHES:
        os.environ.pop(k, None)
    os.environ.update(env)


def record(size, batch, env, flags, params):
    import torch
    from tennis_amd import weights as W
    from tennis_amd.engine import DenseNet121Features
    set_env(env)
    try:
        enc = DenseNet121Features(params, size, max_batch=batch, exact_weights=bool(flags & EXACT))
    finally:
        set_env({})
    stats, _ = enc.profile(torch.from_numpy(W.synthetic_frames_u8(batch, size)).cuda())
    torch.cuda.synchronize()
    del enc
    return [[s["name"], s["launches"], s["flops"], s["bytes"]] for s in stats]


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "encoder_routes.json"))
    args = ap.parse_args()
    from tennis_amd import weights as W
    params = W.make_densenet121_weights(0)
    entries = []
    for size, batch, env, flags in cases():
        fams = record(size, batch, env, flags, params)
        entries.append({"size": size, "batch": batch, "env": env, "flags": flags, "families": fams})
        print(size, batch, env, flags, [f[0] for f in fams], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("[\n" + ",\n".join(json.dumps(e) for e in entries) + "\n]\n")      # (json round-trips a double through repr exactly)
    print(f"{len(entries)} entries -> {args.out}")


if __name__ == "__main__":
    main()
