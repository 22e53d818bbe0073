"""A small on-disk caption dataset in FEATURE mode (data/README.md layout) for the clip-table tests: per split one video whose frames
exist as (empty) files - the dataset only asks whether they exist -, label files, splits/02/<split>.txt, annotations/points.txt +
captions.txt, and one ``.npy`` feature per frame under features/<feats_model>/.  The points are ragged (2 .. 9 frames), two of the
train split overlap, and they are listed out of frame order."""
import os

import numpy as np

WORDS = "the near far player serves hits a forehand backhand return into net wide ace winner long".split()
# (start, end) per split; train: 12 points, points 3 and 4 overlap (frames 20..24 are shared), the last one precedes the others
CLIPS = {"train": [(1, 10), (11, 13), (14, 19), (20, 27), (22, 25), (28, 31), (32, 40), (41, 46), (47, 49), (50, 57), (58, 62), (3, 7)],
         "val": [(1, 6), (4, 13), (14, 16)],
         "test": [(2, 5), (6, 15), (10, 12)]}


def write(root, feature_dim=20, feats_model="0042", seed=3):
    """-> {split: [(pid, video, start, end, caption)]}"""
    from tennis_amd.dataset import TennisSet
    rng = np.random.default_rng(seed)
    os.makedirs(os.path.join(root, "splits", "02"), exist_ok=True)
    os.makedirs(os.path.join(root, "annotations", "labels"), exist_ok=True)
    points, pts_lines, cap_lines = {}, [], []
    for vi, split in enumerate(("train", "val", "test")):
        v = f"V{20 + vi:03d}"
        n = max(e for _, e in CLIPS[split]) + 2
        with open(os.path.join(root, "annotations", "labels", v + ".txt"), "w") as f:
            f.write("".join(f"{fr} OTH\n" for fr in range(n)))
        with open(os.path.join(root, "splits", "02", split + ".txt"), "w") as f:
            f.write("".join(f"{v} {fr}\n" for fr in range(n)))
        for fr in range(n):
            path = os.path.join(root, "frames", v + ".mp4", "0000000000", f"{fr:010d}.jpg")
            os.makedirs(os.path.dirname(path), exist_ok=True)
            open(path, "wb").close()
            feat = TennisSet.get_feature_path(os.path.join(root, "features", feats_model), v, fr)
            os.makedirs(os.path.dirname(feat), exist_ok=True)
            np.save(feat, (np.abs(rng.normal(0, 1, feature_dim)) * 0.5).astype(np.float32))
        points[split] = []
        for i, (a, b) in enumerate(CLIPS[split]):
            pid, cap = f"P{split}{i:02d}", " ".join(rng.choice(WORDS, size=int(rng.integers(2, 9))))
            points[split].append((pid, v, a, b, cap))
            pts_lines.append(f"{pid} {v} {a} {b}")
            cap_lines.append(f"{pid}\t{cap}")
    with open(os.path.join(root, "annotations", "points.txt"), "w") as f:
        f.write("\n".join(pts_lines) + "\n")
    with open(os.path.join(root, "annotations", "captions.txt"), "w") as f:
        f.write("\n".join(cap_lines) + "\n")
    return points
