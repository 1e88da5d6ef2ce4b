"""Batched float64 teacher-forced decode reference on the oracle (oracle/restatement.py).

Given the tokens every decode row was actually fed (the kernel's next_token after each selection, <start> first) and the
row-to-image map, one decoder stack over all rows and positions yields every step's raw scores (V+K+F) at once; the
causal mask makes position i of that stack the oracle's full-recompute decode step i.  The fact indicators are
recomputed per step over the caption buffer up to that step, as the oracle's predict() does (training's indicators see
only the positions before each one: a different rule).
"""
import contextlib
import math

import numpy as np
import torch

from oracle import restatement as R


@contextlib.contextmanager
def float64_default():
    """The oracle allocates with the default dtype (context_indicators, pe_table, attention masks): run it in float64
    and always restore the caller's default."""
    before = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)
    try:
        yield
    finally:
        torch.set_default_dtype(before)


def params64(P):
    return {k: (v.double() if v.is_floating_point() else v) for k, v in P.items()}


def feed_masks(cfg, fed, K):
    """CaptionEmbedder masks of the fed tokens: 0 at <start>, 1 for an entity pointer, 2 for a fact pointer."""
    V = cfg.vocab_size
    m = torch.where(fed >= V, torch.ones_like(fed), torch.zeros_like(fed))
    if cfg.has_facts:
        m = torch.where(fed >= V + K, torch.full_like(fed, 2), m)
    m[:, 0] = 0
    return m


class Fp64Decode:
    """The fp64 oracle of one batch of images (enc_out (B, d, 196), entities (B, K, 5|10), facts (B, F, 3) or None)."""

    def __init__(self, cfg, P, enc_out, entities, facts=None):
        self.cfg, self.P = cfg, params64(P)
        self.entities, self.facts = entities, facts
        self.K = entities.shape[1]
        with float64_default(), torch.no_grad():
            self.enc = enc_out.double()
            self.ee = R.entity_encode(cfg, self.P, entities, facts)
            self.fe = R.fact_encode(self.P, facts, self.ee) if cfg.has_facts else None
            self.mem = R.build_memory(cfg, self.P, self.enc, self.ee, self.fe)

    def scores(self, fed, img, steps=None, first=0):
        """fed: (R, n) int64 tokens row r was fed at positions 0..n-1; img: (R,) image of each row (r // rows_per_sample).
        Returns float64 numpy (R, steps - first, V+K+F): the raw scores of decode steps first..steps-1 (steps <= n)."""
        cfg, P, K = self.cfg, self.P, self.K
        fed = torch.as_tensor(fed, dtype=torch.long).cpu()
        img = torch.as_tensor(img, dtype=torch.long).cpu()
        Rn, n = fed.shape
        steps = n if steps is None else steps
        with float64_default(), torch.no_grad():
            ee = self.ee[img]
            fe = self.fe[img] if self.fe is not None else None
            emb = R.caption_embed(cfg, P, fed, feed_masks(cfg, fed, K), ee, fe)
            x = emb * math.sqrt(cfg.emb_dim) + R.pe_table(n, cfg.emb_dim).unsqueeze(0)
            h = R.decoder_stack(cfg, P, x, self.mem[img])
            out = []
            for i in range(first, steps):
                hh = h[:, i:i + 1]
                if cfg.has_facts:
                    eib, pi = R.context_indicators(cfg, fed[:, :i + 1], self.facts[img], K, 1)
                    sc = R.get_scores(cfg, P, hh, ee, fe, eib, pi)
                else:
                    sc = R.get_scores(cfg, P, hh, ee)
                out.append(sc[:, 0])
            return torch.stack(out, dim=1).numpy()

    def greedy(self, img, max_len):
        """The oracle's own greedy decode of every row (fed its own decisions): [(output list, smallest fp64 margin of
        its decisions)] per row."""
        cfg = self.cfg
        Rn = len(img)
        fed = torch.full((Rn, 1), cfg.start, dtype=torch.long)
        rows = [dict(output=[cfg.pad] * max_len, ptt=[], margin=np.inf, done=False) for _ in range(Rn)]
        for i in range(max_len):
            sc = self.scores(fed, img, i + 1, first=i)[:, 0]
            nxt = torch.full((Rn, 1), cfg.start, dtype=torch.long)
            for r, st in enumerate(rows):
                if st["done"]:
                    continue
                order = np.argsort(-sc[r], kind="stable")[:3]
                top = sc[r][order]
                st["margin"] = min(st["margin"], top[0] - top[1], top[1] - top[2])
                st["output"][i] = int(order[0])
                if order[0] == cfg.end:
                    st["done"] = True
                    continue
                st["ptt"].append(int(order[1]))
                R.loop_cleanup(st["output"], st["ptt"], i)
                nxt[r, 0] = st["output"][i]
            if all(st["done"] for st in rows):
                break
            fed = torch.cat([fed, nxt], dim=1)
        return [(st["output"], st["margin"]) for st in rows]

    def sequence_logprobs(self, seqs, img, max_len):
        """Summed fp64 log-probability of each token list in `seqs` (up to and including <end>), teacher-forced in one
        batch: the oracle's sequence_logprob of every row."""
        toks = [upto_end(s, self.cfg.end) for s in seqs]
        n = max(1, max(len(t) for t in toks))
        fed = torch.full((len(toks), n), self.cfg.start, dtype=torch.long)
        for r, t in enumerate(toks):
            if len(t) > 1:
                fed[r, 1:len(t)] = torch.tensor(t[:-1])
        sc = self.scores(fed, img)
        lsm = log_softmax(sc)
        return [float(sum(lsm[r, i, q] for i, q in enumerate(t))) for r, t in enumerate(toks)]


def log_softmax(sc):
    m = sc.max(axis=-1, keepdims=True)
    return sc - (m + np.log(np.exp(sc - m).sum(axis=-1, keepdims=True)))


def upto_end(seq, end):
    seq = [int(q) for q in seq]
    return seq[:seq.index(end) + 1] if end in seq else seq


def greedy_choices(cfg, sc, max_len):
    """The oracle's predict() decisions on one row's teacher-forced scores sc (steps, Vx), with its own runner-up
    history: (choice per step after the n-gram clean-up, output list after the last step, top-2 and 2nd-3rd margins
    per step).  Stops after <end>."""
    output = [cfg.pad] * max_len
    prev_top_two, choice, margins = [], [], []
    for i in range(sc.shape[0]):
        order = np.argsort(-sc[i], kind="stable")[:3]
        top = sc[i][order]
        m12 = top[0] - top[1]
        out = int(order[0])
        output[i] = out
        if out == cfg.end:
            choice.append(out)
            margins.append(m12)
            break
        prev_top_two.append(int(order[1]))
        R.loop_cleanup(output, prev_top_two, i)
        choice.append(output[i])
        # where the clean-up took the runner-up, the 2nd / 3rd order decides too
        margins.append(m12 if output[i] == out or top.size < 3 else min(m12, top[1] - top[2]))
    return choice, output, margins
