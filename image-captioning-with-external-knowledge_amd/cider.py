"""CIDEr-D on the device: the reward of self-critical training (SelfCriticalStep) and a corpus metric.

The metric is coco-caption's CIDEr-D (Vedantam et al. 2015, "CIDEr: Consensus-based Image Description Evaluation"),
applied to token ids instead of PTB-tokenised words:

* Words of a caption (candidate, reference and corpus captions alike): the tokens before the first <end>, without
  <start>, <pad> and the caller's `ignore` ids.  Removal closes the gap: "a <pad> b" has the bigram "a b", as
  eval.py's joined strings do.  Entity and fact pointer ids (>= V) stay ids.  A row with no <end> uses all its tokens.
* n-grams, n = 1..4, with their counts tf(g) (not normalised).
* Document frequency: df(g) is the number of corpus images whose references, taken together, contain g (an image counts
  once however many of its references contain g).  log_ref_len = log(number of corpus images).
* Vectors: x_n(g) = tf(g) * (log_ref_len - log(max(1, df(g)))); for each n the norm is ||x_n||_2.
* Length: the caption's BIGRAM count.  coco-caption accumulates its length at its n-index 1, i.e. over bigrams; that
  quirk is kept so the numbers agree.
* Similarity with one reference, for each n: s_n = sum over g in the candidate of min(x_n^c(g), x_n^r(g)) * x_n^r(g)
  / (||x_n^c|| ||x_n^r||), 0 if either norm is 0; times exp(-delta^2 / (2 sigma^2)), delta = len_c - len_r, sigma = 6.
* Score: the mean of s_n over n = 1..4, averaged over the image's references, times 10.  Range [0, 10].

Because the definition is on ids, a pointer V + k means "entity slot k", and df pools that slot across images.  The
score equals coco-caption's CIDEr-D on the space-joined id strings; it does NOT equal it on detokenised text (multi-word
entity names, PTB punctuation stripping).  `ignore` gets closer, e.g. with the ids of punctuation.

The df table is built on the host once (numpy) and lives on the device: the distinct n-grams as a sorted array of
128-bit keys (four uint32 ids, unused slots 0xFFFFFFFF, sorted lexicographically as unsigned) with an int32 df each.
The kernel (csrc/cider.hip, ick_cider_d) looks keys up by binary search -- exact and deterministic.
"""
import math

import numpy as np
import torch

from . import ops
from .lib import IckError

NONE = 0xFFFFFFFF
MAX_ID = 2 ** 31 - 1


def _rows3(x, name):
    """(N_img, L) or (N_img, M, L) int64 caption rows -> a (N_img, M, L) numpy array."""
    a = np.asarray(x.detach().cpu() if isinstance(x, torch.Tensor) else x)
    if a.dtype.kind not in "iu":
        raise IckError("%s must hold integer token ids" % name)
    a = a.astype(np.int64, copy=False)
    if a.ndim == 2:
        a = a[:, None, :]
    if a.ndim != 3 or a.shape[0] < 1 or a.shape[1] < 1 or a.shape[2] < 1:
        raise IckError("%s must be (N_img, L) or (N_img, M, L) caption rows" % name)
    return a


def _words(rows, start, end, pad, ignore):
    """rows (R, L) -> (compacted words (R, L) int64, padded with -1, word counts (R,))."""
    R, L = rows.shape
    keep = ~(np.cumsum(rows == end, axis=1) > 0)
    keep &= ~np.isin(rows, np.array([start, pad] + list(ignore), dtype=np.int64))
    bad = keep & ((rows < 0) | (rows >= MAX_ID))
    if bad.any():
        raise IckError("token ids must lie in [0, 2^31 - 1)")
    order = np.argsort(~keep, axis=1, kind="stable")
    comp = np.take_along_axis(rows, order, axis=1)
    W = keep.sum(axis=1)
    comp[np.arange(L)[None, :] >= W[:, None]] = -1
    return comp, W


def df_table(corpus, word_map, ignore=()):
    """The df table of a corpus: (keys (U, 4) uint32, counts (U,) int32, log_ref_len).  corpus: (N_img, L) or
    (N_img, M, L) caption rows, every row of an image one of its references."""
    c = _rows3(corpus, "corpus")
    N_img, M, L = c.shape
    comp, W = _words(c.reshape(-1, L), word_map["<start>"], word_map["<end>"], word_map["<pad>"], ignore)
    img = np.repeat(np.arange(N_img, dtype=np.int64), M)
    keys, owner = [], []
    for n in range(1, 5):
        for i in range(L - n + 1):
            ok = np.nonzero(i + n <= W)[0]
            if ok.size == 0:
                continue
            k = np.full((ok.size, 4), NONE, dtype=np.uint32)
            k[:, :n] = comp[ok, i:i + n]
            keys.append(k)
            owner.append(img[ok])
    if not keys:
        raise IckError("the corpus has no n-grams: every caption is empty")
    k = np.concatenate(keys)
    own = np.concatenate(owner)
    hi = (k[:, 0].astype(np.uint64) << np.uint64(32)) | k[:, 1].astype(np.uint64)
    lo = (k[:, 2].astype(np.uint64) << np.uint64(32)) | k[:, 3].astype(np.uint64)
    order = np.lexsort((own, lo, hi))
    hi, lo, own = hi[order], lo[order], own[order]
    # one entry per (n-gram, image), then the number of images per n-gram
    new_pair = np.ones(hi.size, dtype=bool)
    new_pair[1:] = (hi[1:] != hi[:-1]) | (lo[1:] != lo[:-1]) | (own[1:] != own[:-1])
    hi, lo = hi[new_pair], lo[new_pair]
    new_key = np.ones(hi.size, dtype=bool)
    new_key[1:] = (hi[1:] != hi[:-1]) | (lo[1:] != lo[:-1])
    starts = np.nonzero(new_key)[0]
    counts = np.diff(np.append(starts, hi.size)).astype(np.int32)
    hi, lo = hi[starts], lo[starts]
    out = np.empty((starts.size, 4), dtype=np.uint32)
    out[:, 0], out[:, 1] = (hi >> np.uint64(32)).astype(np.uint32), (hi & np.uint64(NONE)).astype(np.uint32)
    out[:, 2], out[:, 3] = (lo >> np.uint64(32)).astype(np.uint32), (lo & np.uint64(NONE)).astype(np.uint32)
    if out.shape[0] >= 2 ** 31:
        raise IckError("the df table holds more than 2^31 - 1 n-grams")
    return out, counts, math.log(float(N_img))


class CiderD:
    """cider = CiderD(corpus, word_map, sigma=6.0, ignore=())
    rewards = cider(tokens, image_index, refs)       # (N,) float32 on the device, no host synchronisation

    corpus: (N_img, L) or (N_img, M, L) int64 caption rows (CPU or device), e.g. the TRAIN split's captions; the df
    table and log_ref_len are built from it once and kept on the device (`device`, default the current GPU).
    tokens: (N, T) int64 candidate rows; image_index: (N,) row -> image of refs; refs: (B, M, Lr) or (B, L) reference
    captions encoded like the dataset's.  Limits: T, Lr <= 64, M <= 16, at most 16 ignore ids.

    CiderD.from_refs(refs, word_map) takes the df from the scored references themselves (coco-caption's compute_score
    setting): CiderD.from_refs(refs, wm)(cands, arange(B), refs).mean() is its corpus CIDEr-D.
    A SelfCriticalStep given a CiderD as its reward scores on the device (scst(): the SCST-layout launch)."""

    def __init__(self, corpus, word_map, sigma=6.0, ignore=(), device=None):
        if not sigma > 0 or not math.isfinite(sigma):
            raise IckError("sigma must be finite and > 0")
        self.ignore = tuple(int(i) for i in ignore)
        if len(self.ignore) > 16:
            raise IckError("CiderD takes at most 16 ignore ids")
        self.sigma = float(sigma)
        self.start, self.end, self.pad = word_map["<start>"], word_map["<end>"], word_map["<pad>"]
        keys, counts, self.log_ref_len = df_table(corpus, {"<start>": self.start, "<end>": self.end,
                                                            "<pad>": self.pad}, self.ignore)
        self.size = keys.shape[0]
        if device is None:
            device = torch.device("cuda", torch.cuda.current_device())
        # int32 views of the uint32 keys: the kernel reads the bits as unsigned
        self.keys = torch.from_numpy(keys.view(np.int32)).to(device)
        self.counts = torch.from_numpy(counts).to(device)

    @classmethod
    def from_refs(cls, refs, word_map, sigma=6.0, ignore=(), device=None):
        return cls(refs, word_map, sigma=sigma, ignore=ignore, device=device)

    def table(self):
        """The df table on the host: (keys (U, 4) uint32, counts (U,) int32, log_ref_len)."""
        return self.keys.cpu().numpy().view(np.uint32), self.counts.cpu().numpy(), self.log_ref_len

    def _refs(self, refs, dev):
        if not isinstance(refs, torch.Tensor) or refs.dtype != torch.int64:
            raise IckError("refs must be an int64 tensor (B, M, Lr) or (B, L)")
        if refs.dim() == 2:
            refs = refs.unsqueeze(1)
        if refs.dim() != 3:
            raise IckError("refs must be (B, M, Lr) or (B, L)")
        return refs.to(dev).contiguous()

    def _launch(self, tokens, refs, **kw):
        if not isinstance(tokens, torch.Tensor) or tokens.dtype != torch.int64 or tokens.dim() != 2:
            raise IckError("tokens must be an (N, T) int64 tensor")
        dev = self.keys.device
        return ops.cider_d(tokens.to(dev).contiguous(), self._refs(refs, dev), self.keys, self.counts,
                           self.log_ref_len, self.sigma, self.start, self.end, self.pad, self.ignore, **kw)

    def __call__(self, tokens, image_index, refs):
        if not isinstance(image_index, torch.Tensor):
            image_index = torch.as_tensor(image_index)
        return self._launch(tokens, refs, image_index=image_index.to(self.keys.device))[0]

    def scst(self, tokens, refs, num_samples, baseline):
        """SCST layout: tokens rows b * n + j are the samples of image b, followed with baseline="greedy" by the B
        greedy rows.  One launch; returns (rewards (N,), advantages (B * n,)) float32 on the device."""
        return self._launch(tokens, refs, num_samples=num_samples, baseline=baseline)
