"""float64 numpy restatement of the label-smoothed packed cross entropy (ick_packed_ce_smooth).

For a contributing row with scores x[0 .. Vx) (every column of the row, pointer columns included), target t and
lse = logsumexp(x):
    row_loss = (1 - eps) * (lse - x[t]) + eps * (lse - mean(x))
    d row_loss / d x[c] = softmax(x)[c] - (1 - eps) * [c == t] - eps / Vx
A row (b, t) contributes when t < min(decode_len[b], L - 1) and its target caps[b, t + 1] is not <pad> and lies in
[0, Vx).  loss_sum = sum of weight[b] * row_loss, count = the number of contributing rows (unweighted), the gradient of a
row is multiplied by weight[b]; rows that do not contribute have a zero gradient."""
import numpy as np


def contributing(caps, decode_len, pad, Vx):
    """(B, L) bool: the rows that contribute."""
    caps = np.asarray(caps)
    B, L = caps.shape
    keep = np.zeros((B, L), dtype=bool)
    for b in range(B):
        for t in range(min(L - 1, max(int(decode_len[b]), 0))):
            y = int(caps[b, t + 1])
            keep[b, t] = y != pad and 0 <= y < Vx
    return keep


def smoothed_ce(scores, caps, decode_len, pad, eps, weights=None):
    """Unpacked layout: scores (B, L, Vx) -> (loss_sum, count, dscores (B, L, Vx)), all float64."""
    x = np.asarray(scores, dtype=np.float64)
    caps = np.asarray(caps)
    B, L, Vx = x.shape
    w = np.ones(B) if weights is None else np.asarray(weights, dtype=np.float64)
    keep = contributing(caps, decode_len, pad, Vx)
    d = np.zeros_like(x)
    loss, count = 0.0, 0
    for b, t in zip(*np.nonzero(keep)):
        s, y = x[b, t], int(caps[b, t + 1])
        m = s.max()
        lse = m + np.log(np.exp(s - m).sum())
        loss += w[b] * ((1.0 - eps) * (lse - s[y]) + eps * (lse - s.mean()))
        count += 1
        g = np.exp(s - lse) - eps / Vx
        g[y] -= 1.0 - eps
        d[b, t] = w[b] * g
    return loss, count, d


def pack_rows(lengths, L):
    """The packed row list of ick_head_rowmap: rowmap[m] = b * L + t for t < clamp(lengths[b] - 1, 0, L - 1), sample-major."""
    return np.array([b * L + t for b, n in enumerate(np.asarray(lengths).reshape(-1))
                     for t in range(min(max(int(n) - 1, 0), L - 1))], dtype=np.int64)


def smoothed_ce_packed(packed_scores, caps, lengths, pad, eps, weights=None):
    """Packed layout: row m of packed_scores (M', Vx) is position rowmap[m] -> (loss_sum, count, dscores (M', Vx)).  A
    packed row whose target is <pad> (or outside the row) is a zero gradient row that does not count."""
    caps = np.asarray(caps)
    B, L = caps.shape
    rowmap = pack_rows(lengths, L)
    xp = np.asarray(packed_scores, dtype=np.float64)
    assert xp.shape[0] == rowmap.size
    full = np.zeros((B * L, xp.shape[1]))
    full[rowmap] = xp
    dl = np.asarray(lengths).reshape(-1) - 1
    loss, count, d = smoothed_ce(full.reshape(B, L, -1), caps, dl, pad, eps, weights)
    return loss, count, d.reshape(B * L, -1)[rowmap]
