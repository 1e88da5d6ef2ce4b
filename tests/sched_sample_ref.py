"""numpy restatement of the scheduled-sampling mix kernel (csrc/sched_sample.hip, ick_sched_sample_mix), written from its
definition (include/ick_amd.h): the coin, the Gumbel-max draw, the banned columns and the token / mask
rule.  Philox-4x32-10 is tests/sample_ref.py's.

With n_b = clamp(lengths[b] - 1, 0, L - 1), position (b, q) is eligible when 1 <= q <= n_b - 1 and packed row
rowstart[b] + q - 1 predicts its token; rowstart is the exclusive scan of the n_b."""
import numpy as np

from sample_ref import MASK, philox4x32_10

COIN_QUAD = 0xFFFFFFFF


def key_of(seed):
    seed &= (1 << 64) - 1
    return seed & MASK, seed >> 32


def valid_rows(lengths, L):
    """-> (n_b (B,), rowstart (B + 1,)) from the caption lengths."""
    n = np.clip(np.asarray(lengths, dtype=np.int64).reshape(-1) - 1, 0, L - 1)
    return n, np.concatenate([[0], np.cumsum(n)]).astype(np.int64)


def coin_numerators(seed, step, bs, qs):
    """(x >> 8) + 0.5 of the coins of positions (bs[i], qs[i]), float64 (exact): replaced iff it is < prob * 2^24."""
    bs, qs = np.asarray(bs, dtype=np.uint64), np.asarray(qs, dtype=np.uint64)
    ctr = np.stack([np.full_like(bs, COIN_QUAD), np.full_like(bs, step & MASK), (qs - np.uint64(1)) & np.uint64(MASK), bs],
                   axis=1)
    x = philox4x32_10(ctr, key_of(seed))[:, 0]
    return (x >> 8).astype(np.float64) + 0.5


def coins(seed, step, bs, qs, prob):
    return coin_numerators(seed, step, bs, qs) < float(prob) * 16777216.0


def noise(seed, step, b, q, ncols, dtype=np.float32):
    """Gumbel noise of columns 0 .. ncols - 1 at position (b, q): sample.hip's function of element c & 3 of
    Philox(ctr = (c >> 2, step, q - 1, b)), in fp32 like the kernel or in float64."""
    quads = np.arange((ncols + 3) // 4, dtype=np.uint64)
    ctr = np.stack([quads, np.full_like(quads, step & MASK), np.full_like(quads, q - 1), np.full_like(quads, b)], axis=1)
    x = philox4x32_10(ctr, key_of(seed)).reshape(-1)[:ncols]
    u = ((x >> 8).astype(dtype) + dtype(0.5)) * dtype(2.0 ** -24)
    u = np.minimum(u, dtype(1.0 - 2.0 ** -24))
    return -np.log(-np.log(u))


def draw(s, banned, g=None, T=1.0, dtype=np.float32):
    """(column, margin) of one row: the first maximum of s (argmax mode, g None) or of s / T + g over the columns that
    are not banned; margin = the winner's lead over the runner-up."""
    s = np.asarray(s, dtype=dtype)
    v = s.copy() if g is None else (s / dtype(T) + g.astype(dtype)).astype(dtype)
    ok = np.ones(v.shape, dtype=bool)
    for c in banned:
        if 0 <= c < v.size:
            ok[c] = False
    v = np.where(ok, v, -np.inf)
    tok = int(np.argmax(v))             # first maximum: ties to the lower column
    rest = np.delete(v, tok)
    return tok, float(v[tok] - rest.max()) if rest.size else float("inf")


def token_mask(c, V, K):
    return 0 if c < V else (1 if c < V + K else 2)


def mix(rows, lengths, caps, masks, V, K, F, start, pad, prob, T, seed, step, argmax, dtype=np.float32):
    """rows: (M', >= Vx) packed score rows (only those of replaced positions are read).  -> (captions_in, masks_in int64,
    replaced int32, margins {(b, q): the draw's margin})."""
    caps, masks = np.asarray(caps, dtype=np.int64), np.asarray(masks, dtype=np.int64)
    B, L = caps.shape
    Vx = V + K + F
    n, rowstart = valid_rows(lengths, L)
    caps_in, masks_in = caps.copy(), masks.copy()
    replaced = np.zeros((B, L), dtype=np.int32)
    margins = {}
    el = [(b, q) for b in range(B) for q in range(1, int(n[b]))]      # 1 <= q <= n_b - 1
    if not el:
        return caps_in, masks_in, replaced, margins
    hit = coins(seed, step, [b for b, _ in el], [q for _, q in el], prob)
    for (b, q), h in zip(el, hit):
        if not h:
            continue
        s = np.asarray(rows[rowstart[b] + q - 1])[:Vx]
        g = None if argmax else noise(seed, step, b, q, Vx, dtype)
        c, margins[(b, q)] = draw(s, (start, pad), g, T, dtype)
        caps_in[b, q], masks_in[b, q], replaced[b, q] = c, token_mask(c, V, K), 1
    return caps_in, masks_in, replaced, margins
