"""BLEU-1..4, ROUGE-L and pointer precision / recall on the device: corpus metrics of generated captions, and, mixed
with CIDEr-D, rewards of self-critical training (SelfCriticalStep).

The metrics are coco-caption's (bleu_scorer with option="closest"; Rouge with beta = 1.2), applied to token ids instead
of PTB-tokenised words.  The definitions, on token ids, are the contract (include/ick_amd.h states the same):

* Words of a caption: CiderD's words exactly (cider.py; the kernels share the code): the tokens before the first
  <end>, without <start>, <pad> and up to 16 `ignore` ids.  Removal closes the gap.  A row without <end> uses all its
  tokens.  Ids >= V stay ids.  c = the candidate's word count, l_m = the word count of its reference m.
  Limits: T, Lr <= 64, M <= 16.
* BLEU components per candidate, n = 1..4:
    guess_n   = max(0, c - n + 1)
    correct_n = sum over the distinct candidate n-grams g of min(count_c(g), max_m count_m(g))
    testlen   = c
    reflen    = the l_m that minimises (|l_m - c|, l_m)
* Sentence BLEU-n = (prod_{k<=n} (correct_k + 1e-15) / (guess_k + 1e-9)) ** (1/n); if ratio = (testlen + 1e-15) /
  (reflen + 1e-9) < 1, times exp(1 - 1/ratio).
* Corpus BLEU-n: the same formula on the sums of the ten components over all scored captions.
* ROUGE-L: P = max_m LCS(c, r_m) / c, R = max_m LCS(c, r_m) / l_m (an empty reference contributes 0 where coco-caption
  divides by zero); the score is (1 + beta^2) P R / (R + beta^2 P), 0 when P or R is 0 or c = 0.  Corpus: the mean over
  captions.
* Pointer precision / recall, with pointer_base = V.  Per caption: generated = the number of distinct ids >= V among
  the candidate's words, reference = the number of distinct ids >= V in the union of its references' words, hits = the
  size of the intersection.  Corpus: precision = sum hits / sum generated, recall = sum hits / sum reference, each 0
  when its denominator is 0.

Because the definitions are on ids, the scores equal coco-caption's on the space-joined id strings; they do NOT equal
them on detokenised text (multi-word entity names, PTB punctuation stripping); `ignore` gets closer, e.g. with the ids
of punctuation.  The pointer counts are the id-level counterpart of the news variant's named-entity precision / recall
in its "exact" mode: a pointer V + k is "entity slot k of this image", where the script compares the entity strings spaCy
finds in the two texts.  METEOR (WordNet, a Java aligner) and spaCy's entity extraction are not provided.

The kernel (csrc/metrics.hip, ick_caption_metrics) writes per-row results; ick_caption_metric_sums adds them up on the
device in a fixed order, and result() turns totals into the corpus numbers on the host -- the one synchronisation.
"""
import collections
import math

import torch

from . import ops
from .lib import IckError

CaptionMetricRows = collections.namedtuple("CaptionMetricRows", "counts bleu rouge_l pointers")
CaptionMetricRows.__doc__ = """Per-row device tensors: counts (N, 10) int32 = guess1..4, correct1..4, testlen, reflen;
bleu (N, 4) float32 sentence BLEU-1..4; rouge_l (N,) float32; pointers (N, 3) int32 = hits, generated, reference.  A row
whose image_index was out of range holds NaN floats and zero counts."""


class CaptionMetricTotals(collections.namedtuple("CaptionMetricTotals", "sums rouge_sum")):
    """Device totals: sums (14,) int64 = the ten BLEU components, pointer hits / generated / reference and the number
    of captions; rouge_sum (1,) float64.  a + b adds two batches' totals on the device."""
    __slots__ = ()

    def __add__(self, other):
        if not isinstance(other, CaptionMetricTotals):
            return NotImplemented
        return CaptionMetricTotals(self.sums + other.sums, self.rouge_sum + other.rouge_sum)


def corpus_bleu(comps):
    """[Bleu_1..Bleu_4] from the ten summed components (guess1..4, correct1..4, testlen, reflen), float64."""
    guess, correct, testlen, reflen = comps[0:4], comps[4:8], comps[8], comps[9]
    ratio = (testlen + 1e-15) / (reflen + 1e-9)
    bp = math.exp(1.0 - 1.0 / ratio) if ratio < 1.0 else 1.0
    out, p = [], 1.0
    for k in range(4):
        p *= (float(correct[k]) + 1e-15) / (float(guess[k]) + 1e-9)
        out.append(p ** (1.0 / (k + 1)) * bp)
    return out


def _tokens_ok(tokens):
    if not isinstance(tokens, torch.Tensor) or tokens.dtype != torch.int64 or tokens.dim() != 2:
        raise IckError("tokens must be an (N, T) int64 tensor")


class CaptionMetrics:
    """m = CaptionMetrics(word_map, ignore=(), pointer_base=None, beta=1.2, device=None)
    rows = m(tokens, image_index, refs)          # CaptionMetricRows on the device, no host synchronisation
    totals = m.totals(rows)                      # CaptionMetricTotals on the device; totals + totals adds batches
    CaptionMetrics.result(totals)                # dict: Bleu_1..Bleu_4, ROUGE_L, pointer_precision, pointer_recall, captions

    tokens: (N, T) int64 candidate rows; image_index: (N,) row -> image of refs; refs: (B, M, Lr) or (B, L) int64
    reference captions encoded like the dataset's.  pointer_base: the first pointer id (V = len(word_map)); None: no
    pointer counts (zeros).  device: where the tensors go (default: the candidates' device, else the current GPU).
    m.reward(...) makes a MetricReward for SelfCriticalStep."""

    def __init__(self, word_map, ignore=(), pointer_base=None, beta=1.2, device=None):
        try:
            self.start, self.end, self.pad = int(word_map["<start>"]), int(word_map["<end>"]), int(word_map["<pad>"])
        except (KeyError, TypeError):
            raise IckError("word_map must map <start>, <end> and <pad> to their ids")
        self.ignore = tuple(int(i) for i in ignore)
        if len(self.ignore) > 16:
            raise IckError("CaptionMetrics takes at most 16 ignore ids")
        if not isinstance(beta, (int, float)) or not beta > 0 or not math.isfinite(beta):
            raise IckError("beta must be finite and > 0")
        if pointer_base is not None and (isinstance(pointer_base, bool) or not isinstance(pointer_base, int) or
                                         not 0 <= pointer_base < 2 ** 31 - 1):
            raise IckError("pointer_base must be None or an id in [0, 2^31 - 1)")
        self.beta = float(beta)
        self.pointer_base = -1 if pointer_base is None else pointer_base
        self.device = torch.device(device) if device is not None else None

    def _device(self, tokens):
        if self.device is not None:
            return self.device
        return tokens.device if tokens.is_cuda else torch.device("cuda", torch.cuda.current_device())

    @staticmethod
    def _refs(refs, dev):
        if not isinstance(refs, torch.Tensor) or refs.dtype != torch.int64:
            raise IckError("refs must be an int64 tensor (B, M, Lr) or (B, L)")
        if refs.dim() == 2:
            refs = refs.unsqueeze(1)
        if refs.dim() != 3:
            raise IckError("refs must be (B, M, Lr) or (B, L)")
        return refs.to(dev).contiguous()

    def _launch(self, tokens, refs, **kw):
        _tokens_ok(tokens)
        dev = self._device(tokens)
        return ops.caption_metrics(tokens.to(dev).contiguous(), self._refs(refs, dev), self.start, self.end, self.pad,
                                   self.ignore, self.pointer_base, self.beta, **kw)

    def __call__(self, tokens, image_index, refs):
        _tokens_ok(tokens)
        if not isinstance(image_index, torch.Tensor):
            image_index = torch.as_tensor(image_index)
        out = self._launch(tokens, refs, image_index=image_index.to(self._device(tokens)))
        return CaptionMetricRows(*out[:4])

    def totals(self, rows):
        """The device totals of one batch's rows (rows of an out-of-range image_index are skipped)."""
        return CaptionMetricTotals(*ops.caption_metric_sums(rows.counts, rows.rouge_l, rows.pointers))

    @staticmethod
    def result(totals):
        """Corpus numbers from totals, in float64 on the host (this reads the totals: one synchronisation)."""
        s = [int(x) for x in totals.sums.tolist()]
        rouge = float(totals.rouge_sum.tolist()[0])
        bleu = corpus_bleu(s[:10]) if s[13] else [0.0] * 4
        hits, gen, ref, n = s[10], s[11], s[12], s[13]
        out = {"Bleu_%d" % (k + 1): bleu[k] for k in range(4)}
        out.update(ROUGE_L=rouge / n if n else 0.0, pointer_precision=hits / gen if gen else 0.0,
                   pointer_recall=hits / ref if ref else 0.0, captions=n)
        return out

    def reward(self, cider=None, cider_weight=1.0, bleu=(0, 0, 0, 0), rouge_l=0.0):
        """A reward cider_weight * CIDEr-D + sum_n bleu[n-1] * BLEU-n + rouge_l * ROUGE-L (sentence scores) for
        SelfCriticalStep; cider: a cider.CiderD, or None for no CIDEr-D term."""
        return MetricReward(self, cider, cider_weight, bleu, rouge_l)


class MetricReward:
    """reward = metrics.reward(cider=CiderD(...), cider_weight=1.0, bleu=(0, 0, 0, 0.5), rouge_l=0.0)
    reward(tokens, image_index, refs) -> (N,) float32 rewards on the device (general mode);
    reward.scst(tokens, refs, num_samples, baseline) -> (rewards (N,), advantages (B * n,)), the SCST layout of
    CiderD.scst: the CiderD launch (if any), then ick_caption_metrics on its rewards.  A SelfCriticalStep takes it as a
    device reward (refs= required, nothing copied to the host).  The rewards are w_base * cider + w_b1 * bleu1 + .. +
    w_rouge * rouge evaluated in fp32 in this order, so cider_weight=1 with every other weight 0 gives CiderD's bits."""

    def __init__(self, metrics, cider=None, cider_weight=1.0, bleu=(0, 0, 0, 0), rouge_l=0.0):
        from .cider import CiderD
        if not isinstance(metrics, CaptionMetrics):
            raise IckError("MetricReward needs a CaptionMetrics")
        if cider is not None and not isinstance(cider, CiderD):
            raise IckError("cider must be a cider.CiderD or None")
        try:
            bleu = tuple(float(b) for b in bleu)
            w = (float(cider_weight),) + bleu + (float(rouge_l),)
        except (TypeError, ValueError):
            raise IckError("the reward weights must be numbers: cider_weight, bleu = four weights, rouge_l")
        if len(bleu) != 4:
            raise IckError("bleu takes four weights, of BLEU-1..BLEU-4")
        if not all(math.isfinite(x) for x in w):
            raise IckError("the reward weights must be finite")
        if not any(w[1:]) and (cider is None or w[0] == 0.0):
            raise IckError("a reward needs a non-zero weight (with cider=None the CIDEr-D term is absent)")
        if cider is not None and (cider.start, cider.end, cider.pad, cider.ignore) != \
                (metrics.start, metrics.end, metrics.pad, metrics.ignore):
            raise IckError("the CiderD and the CaptionMetrics must agree on <start>, <end>, <pad> and ignore")
        self.metrics, self.cider, self.weights = metrics, cider, w

    def __call__(self, tokens, image_index, refs):
        _tokens_ok(tokens)
        if not isinstance(image_index, torch.Tensor):
            image_index = torch.as_tensor(image_index)
        base = self.cider(tokens, image_index, refs) if self.cider is not None else None
        dev = base.device if base is not None else self.metrics._device(tokens)
        m = self.metrics
        return ops.caption_metrics(tokens.to(dev).contiguous(), m._refs(refs, dev), m.start, m.end, m.pad, m.ignore,
                                   m.pointer_base, m.beta, image_index=image_index.to(dev), base_rewards=base,
                                   weights=self.weights)[4]

    def scst(self, tokens, refs, num_samples, baseline):
        """SCST layout (CiderD.scst's): returns (rewards (N,), advantages (B * n,)) float32 on the device."""
        _tokens_ok(tokens)
        base = self.cider.scst(tokens, refs, num_samples, baseline)[0] if self.cider is not None else None
        dev = base.device if base is not None else self.metrics._device(tokens)
        m = self.metrics
        out = ops.caption_metrics(tokens.to(dev).contiguous(), m._refs(refs, dev), m.start, m.end, m.pad, m.ignore,
                                  m.pointer_base, m.beta, num_samples=num_samples, baseline=baseline,
                                  base_rewards=base, weights=self.weights)
        return out[4], out[5]
