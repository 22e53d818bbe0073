"""Reference for the captioner's attention weights (tests only), built on the unchanged oracle ``oracle.gnmt_np``.

``AttentionDecoder`` is the oracle's ``Decoder`` whose ``step`` also keeps the step's attention distribution, recomputed in float64
from exactly what ``Decoder.step`` forms it from: the new first-layer state (``new_states[0]``), the memory, the key weight and the
mask - query scaled by 1/sqrt(H), masked scores -> -1e18, softmax, times mask (gluonnlp's scaled-Luong cell as the oracle restates it).

A hypothesis' attention in a beam search depends only on its own token prefix: the decoder row that emits token i + 1 carries the
states its ancestors left, which are the states of teacher forcing the prefix.  So the reference for a beam-search alignment is
``teacher_forcing`` of the hypothesis' own tokens (``hypothesis_alignments``); tests/test_cpu_gnmt_attention.py pins that argument
against the oracle's own beam search (``ancestry_weights``)."""
from __future__ import annotations

import numpy as np

from oracle import gnmt_np as gn


class AttentionDecoder(gn.Decoder):
    """``record=True`` also keeps, per step, what ``ancestry_weights`` needs: the tokens and attention input the step was given, the
    context it returned and its weights."""

    def __init__(self, *args, record=False, **kwargs):
        super().__init__(*args, **kwargs)
        self.record, self.trace = record, []

    def init_state(self, mem, enc_states, valid_length):
        out = super().init_state(mem, enc_states, valid_length)
        wk = self.p[self.pre + "dec_attention_key_weight"].astype(np.float64)
        self.keyproj64 = mem.astype(np.float64) @ wk.T
        self.trace = []
        return out

    def step(self, tokens, rnn_states, att, rows):
        logp, new_states, ctx = super().step(tokens, rnn_states, att, rows)
        q = new_states[0].astype(np.float64) / np.sqrt(np.float64(self.h))
        score = np.einsum("rh,rth->rt", q, self.keyproj64[rows])
        m = self.mask[rows]
        score = np.where(m, score, np.float64(gn.NEG))
        e = np.exp(score - score.max(axis=-1, keepdims=True))
        self.last_weights = e / e.sum(axis=-1, keepdims=True) * m          # (R, T) float64
        if self.record:
            self.trace.append((np.asarray(tokens).copy(), att.copy(), ctx.copy(), self.last_weights.copy()))
        return logp, new_states, ctx


def teacher_forcing(dec: AttentionDecoder, mem, enc_states, valid_length, tgt, rows=None):
    """``gn.decode_seq`` with the weights: tgt (R, L) ids (negative ids are fed as 0, like the oracle) -> (logits (R, L, V) float32,
    weights (R, L, T) float64).  ``rows`` (R,) names each target row's clip (default: row r reads clip r)."""
    rows = np.arange(mem.shape[0]) if rows is None else np.asarray(rows)
    rnn_states, att = dec.init_state(mem, enc_states, valid_length)
    rnn_states, att = [s[rows] for s in rnn_states], att[rows]
    logits, weights = [], []
    for i in range(tgt.shape[1]):
        _, rnn_states, att = dec.step(np.maximum(tgt[:, i], 0), rnn_states, att, rows)
        logits.append(dec.last_logits)
        weights.append(dec.last_weights)
    return np.stack(logits, axis=1), np.stack(weights, axis=1)


def emitted_rows(vlen, max_length):
    """How many attention rows a hypothesis of valid length ``vlen`` has: one per token a decoder step emitted.  Tokens 1 .. vlen - 1
    were emitted, unless the search ran to ``max_length`` with the beam alive: then the sampler appended the closing <eos>
    (vlen = max_length + 2) and only max_length steps ran."""
    return np.minimum(np.asarray(vlen) - 1, max_length)


def hypothesis_alignments(dec: AttentionDecoder, mem, enc_states, valid_length, samples, vlen, max_length):
    """Reference alignments of the hypotheses ``samples`` (B, beam, n) / ``vlen`` (B, beam) of a beam search: teacher forcing of each
    hypothesis' own tokens -> (weights (B, beam, n - 1, T) float64 with zeros in the rows no decoder step emitted, rows (B, beam))."""
    B, beam, n = samples.shape
    w = teacher_forcing(dec, mem, enc_states, valid_length, samples.reshape(B * beam, n)[:, :n - 1], np.repeat(np.arange(B), beam))[1]
    w = w.reshape(B, beam, n - 1, -1)
    nrow = emitted_rows(vlen, max_length)
    w[np.arange(n - 1)[None, None, :] >= nrow[:, :, None]] = 0.0
    return w, nrow


def ancestry_weights(dec: AttentionDecoder, samples, vlen, beam, max_length):
    """The oracle's OWN per-step weights along each final hypothesis' ancestry, from the trace of ``gn.beam_search(dec, ...)`` run
    with ``record=True``: the ancestor at step i is the row of the clip that was fed the hypothesis' token i and, from step 1 on, the
    context its ancestor of step i - 1 returned (the sampler re-gathers the states by parent beam).  At step 0 every row of a clip
    is the same <bos> hypothesis.  -> list over (b, k) of (rows, T) arrays, rows = ``emitted_rows``."""
    B = samples.shape[0]
    nrow = emitted_rows(vlen, max_length)
    out = {}
    for b in range(B):
        for k in range(beam):
            r, ws = b * beam, []
            for i in range(int(nrow[b, k])):
                tok, att, ctx, w = dec.trace[i]
                if i:
                    prev_ctx = dec.trace[i - 1][2][r]
                    cand = [c for c in range(b * beam, (b + 1) * beam)
                            if tok[c] == samples[b, k, i] and np.array_equal(att[c], prev_ctx)]
                    assert cand, (b, k, i)
                    r = cand[0]
                ws.append(w[r])
            out[(b, k)] = np.stack(ws) if ws else np.zeros((0, dec.mask.shape[1]))
    return out
