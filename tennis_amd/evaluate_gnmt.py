"""Captioner evaluation driver - counterpart of reference evaluate_gnmt.py: load the best parameters of a model id
(``valid_best.params``, else the newest epoch file) and report teacher-forced loss, perplexity and BLEU of the beam-search
translations on the validation and test splits, writing the sentences out (evaluate_gnmt.py:196-258; same flag names as
train_gnmt).  Feature mode (``--feats_model``): the frame features are the inputs.  Frame mode (no ``--feats_model``): the points'
frames go through the backbone inside the model, whose parameters the checkpoint of a frame-mode training run holds.
``--save_alignments`` (ours): also write ``best_{valid,test}_alignments.npz``, the best beam's attention weights per written word over
the clip's source steps with each step's (video, frame number) (``captions.save_alignments``)."""
from __future__ import annotations

import math
import os

from .captions import bucketed_batches, clip_frame_ids, evaluate, save_alignments, write_sentences
from .metrics.bleu import compute_bleu
from .train_gnmt import build, require_feature_mode
from .train_gnmt import build_parser as _train_parser


def build_parser():
    """train_gnmt's flags plus ``--save_alignments``."""
    p = _train_parser()
    p.add_argument("--save_alignments", action="store_true",
                   help="write best_{valid,test}_alignments.npz next to best_{valid,test}_out.txt: the decoder's attention weights of "
                        "every written word over the clip's source steps, their arg-max step and each step's (video, frame)")
    return p


def main(argv=None):
    flags = build_parser().parse_args(argv)
    require_feature_mode(flags)
    data_train, data_val, data_test, model, translator = build(flags)
    exp = os.path.join(flags.root, flags.model_id)
    path = os.path.join(exp, "valid_best.params")
    if not os.path.exists(path):
        files = sorted(f for f in os.listdir(exp) if f.endswith(".params")) if os.path.isdir(exp) else []
        if not files:
            raise FileNotFoundError(f"no parameter file under {exp}")
        path = os.path.join(exp, files[-1])
    model.load_parameters(path)
    print("Loaded params: {}".format(path))
    out = {}
    for name, ds in (("valid", data_val), ("test", data_test)):
        table, rows = (None, None)
        if flags.feats_on_device:          # the split's features read once, uploaded once; encode_rows gathers every batch's clips
            from .captions import upload_clip_table
            table, rows = upload_clip_table(ds)
        records = [] if flags.save_alignments else None
        loss, sents = evaluate(bucketed_batches(ds, flags.test_batch_size, flags.num_buckets, rows=rows), model, translator, data_train,
                               table=table, alignments=records)
        bleu = compute_bleu([ds.get_captions(split=True)], sents)[0]
        print("Best model {} Loss={:.4f}, {} ppl={:.4f}, {} bleu={:.2f}".format(name, loss, name, math.exp(min(loss, 50.0)), name, bleu * 100))
        write_sentences(sents, os.path.join(exp, "best_{}_out.txt".format(name)))
        if records is not None:
            save_alignments(os.path.join(exp, "best_{}_alignments.npz".format(name)), records, clip_frame_ids(ds))
        out[name] = (loss, bleu)
    return out


if __name__ == "__main__":
    main()
