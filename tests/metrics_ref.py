"""Plain-Python float64 restatement of the caption metrics on token ids (the definitions in ick_amd/metrics.py), written
from those definitions alone: Counter n-grams, a textbook LCS table, sets of pointer ids.  The kernel is held to it.

words (cider_ref.words) -> per-caption BLEU components, sentence BLEU-1..4, ROUGE-L, pointer counts -> corpus results
from the summed components -> the reward combination and the SCST advantages."""
import math
from collections import Counter

from cider_ref import words

BETA = 1.2


def ngram_counts(ws, n):
    return Counter(tuple(ws[i:i + n]) for i in range(len(ws) - n + 1))


def components(cand_w, refs_w):
    """[guess1..4, correct1..4, testlen, reflen] of a candidate's words against its references' words."""
    c = len(cand_w)
    guess, correct = [], []
    for n in range(1, 5):
        cc = ngram_counts(cand_w, n)
        rc = [ngram_counts(r, n) for r in refs_w]
        guess.append(max(0, c - n + 1))
        correct.append(sum(min(k, max(r[g] for r in rc)) for g, k in cc.items()))
    reflen = min(((abs(len(r) - c), len(r)) for r in refs_w))[1]
    return guess + correct + [c, reflen]


def bleu_from(comps):
    """BLEU-1..4 from ten components (one caption's: sentence BLEU; the sums over captions: corpus BLEU)."""
    guess, correct, testlen, reflen = comps[0:4], comps[4:8], comps[8], comps[9]
    ratio = (testlen + 1e-15) / (reflen + 1e-9)
    out, p = [], 1.0
    for n in range(1, 5):
        p *= (correct[n - 1] + 1e-15) / (guess[n - 1] + 1e-9)
        b = p ** (1.0 / n)
        if ratio < 1:
            b *= math.exp(1 - 1 / ratio)
        out.append(b)
    return out


def lcs(a, b):
    """Length of the longest common subsequence (the textbook table)."""
    t = [[0] * (len(b) + 1) for _ in range(len(a) + 1)]
    for i in range(1, len(a) + 1):
        for j in range(1, len(b) + 1):
            t[i][j] = t[i - 1][j - 1] + 1 if a[i - 1] == b[j - 1] else max(t[i - 1][j], t[i][j - 1])
    return t[len(a)][len(b)]


def rouge_l(cand_w, refs_w, beta=BETA):
    c = len(cand_w)
    if c == 0:
        return 0.0
    ls = [lcs(cand_w, r) for r in refs_w]
    P = max(ls) / c
    R = max((l / len(r) if len(r) else 0.0) for l, r in zip(ls, refs_w))
    if P == 0 or R == 0:
        return 0.0
    return (1 + beta ** 2) * P * R / (R + beta ** 2 * P)


def pointer_counts(cand_w, refs_w, pointer_base):
    """[hits, generated, reference]; pointer_base None: zeros."""
    if pointer_base is None:
        return [0, 0, 0]
    gen = {w for w in cand_w if w >= pointer_base}
    ref = {w for r in refs_w for w in r if w >= pointer_base}
    return [len(gen & ref), len(gen), len(ref)]


class Row:
    def __init__(self, counts, bleu, rouge, pointers):
        self.counts, self.bleu, self.rouge_l, self.pointers = counts, bleu, rouge, pointers


def caption(cand, refs, start, end, pad, ignore=(), pointer_base=None, beta=BETA):
    """One candidate row against the reference rows of its image."""
    cw = words(cand, start, end, pad, ignore)
    rw = [words(r, start, end, pad, ignore) for r in refs]
    comps = components(cw, rw)
    return Row(comps, bleu_from(comps), rouge_l(cw, rw, beta), pointer_counts(cw, rw, pointer_base))


def caption_rows(tokens, image_index, refs, start, end, pad, ignore=(), pointer_base=None, beta=BETA):
    """Rows tokens[i] against refs[image_index[i]] (refs: per image, a list of rows)."""
    return [caption(t, refs[int(b)], start, end, pad, ignore, pointer_base, beta) for t, b in zip(tokens, image_index)]


def corpus(rows):
    """The corpus result of a list of Row: the dict CaptionMetrics.result returns."""
    n = len(rows)
    sums = [sum(r.counts[k] for r in rows) for k in range(10)]
    hits, gen, ref = (sum(r.pointers[k] for r in rows) for k in range(3))
    bleu = bleu_from(sums) if n else [0.0] * 4
    out = {"Bleu_%d" % (k + 1): bleu[k] for k in range(4)}
    out["ROUGE_L"] = sum(r.rouge_l for r in rows) / n if n else 0.0
    out["pointer_precision"] = hits / gen if gen else 0.0
    out["pointer_recall"] = hits / ref if ref else 0.0
    out["captions"] = n
    return out


def reward(row, weights, base=None):
    """w_base * base + w_b1 * bleu1 + .. + w_b4 * bleu4 + w_rouge * rouge; base None: no first term."""
    r = 0.0 if base is None else weights[0] * base
    for k in range(4):
        r += weights[1 + k] * row.bleu[k]
    return r + weights[5] * row.rouge_l


def advantages(rewards, B, n, baseline):
    """rewards: B * n sample rewards (row b * n + j), then with "greedy" the B greedy rewards."""
    out = []
    for b in range(B):
        r = rewards[b * n:(b + 1) * n]
        for j in range(n):
            base = rewards[B * n + b] if baseline == "greedy" else (sum(r) - r[j]) / (n - 1)
            out.append(r[j] - base)
    return out
