"""numpy restatement of caption scoring (ick_row_logprob_rank / ick_caption_score_sums): the target's log-probability,
its rank in a stable descending sort, the row's argmax, the validity rule and the rank interval under a score error."""
import numpy as np


def is_valid(target, pad, Vx):
    """packed_ce_rows_kernel's rule: a <pad> target or one outside [0, Vx) does not count."""
    return target != pad and 0 <= target < Vx


def row_stats(s, target):
    """(log-probability, stable rank, argmax) of one score row s (Vx,) for column `target`.  The rank is the target's
    place in a stable descending sort: columns with a higher score, or an equal score and a lower index, come first."""
    s = np.asarray(s)
    w = s.astype(np.float64)
    m = w.max()
    lse = m + np.log(np.exp(w - m).sum())
    st = s[target]
    rank = int((s > st).sum() + (s[:target] == st).sum())
    return float(w[target] - lse), rank, int(np.argmax(s))       # np.argmax: the lowest index of the maximum


def rank_interval(s, target, eps):
    """[lo, hi] that holds the rank of `target` in every row whose scores lie within eps / 2 of s: columns more than
    eps above the target are certainly ahead, columns more than eps below it certainly behind."""
    s = np.asarray(s, dtype=np.float64)
    st = s[target]
    return int((s > st + eps).sum()), int((s >= st - eps).sum()) - 1


def score_batch(scores, captions, lengths, pad, top_k=5, eps=None):
    """Everything score_captions returns, from LOGICAL scores (R, L, Vx) (any row past a caption is ignored), captions
    (R, L) and lengths (R,): dict of token_log_probs / rank / best (R, L-1) with 0 / -1 / -1 fills, log_prob (R,) summed
    in position order, tokens (R,), the four totals, and with eps the interval bounds lo / hi (R, L-1; -1 where unused)
    and the top-two margin of every scored row."""
    scores, captions = np.asarray(scores), np.asarray(captions)
    R, L, Vx = scores.shape
    T = L - 1
    out = dict(token_log_probs=np.zeros((R, T)), rank=-np.ones((R, T), np.int64), best=-np.ones((R, T), np.int64),
               lo=-np.ones((R, T), np.int64), hi=-np.ones((R, T), np.int64), margin=np.zeros((R, T)),
               log_prob=np.zeros(R), tokens=np.zeros(R, np.int64))
    for r in range(R):
        n = int(min(T, max(0, int(lengths[r]) - 1)))
        for t in range(n):
            tg = int(captions[r, t + 1])
            if not is_valid(tg, pad, Vx):
                continue
            lp, rk, bi = row_stats(scores[r, t], tg)
            out["token_log_probs"][r, t], out["rank"][r, t], out["best"][r, t] = lp, rk, bi
            out["log_prob"][r] += lp
            out["tokens"][r] += 1
            if eps is not None:
                out["lo"][r, t], out["hi"][r, t] = rank_interval(scores[r, t], tg, eps)
                top = np.sort(scores[r, t].astype(np.float64))[-2:]
                out["margin"][r, t] = top[-1] - top[0] if Vx > 1 else np.inf
    ok = out["rank"] >= 0
    out["loss_sum"] = -out["token_log_probs"][ok].sum()
    out["count"] = int(ok.sum())
    out["top1_hits"] = int((out["rank"][ok] == 0).sum())
    out["topk_hits"] = int((out["rank"][ok] < top_k).sum())
    return out
