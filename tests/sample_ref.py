"""numpy restatement of the sampled selection of DecoderTransformer.predict_sample (csrc/sample.hip): Philox-4x32-10,
the Gumbel noise, the top-k / top-p kept set and the draw, written from the rules in the docstring / DESIGN.md."""
import numpy as np

M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
MASK = 0xFFFFFFFF


def philox4x32_10(ctr, key):
    """ctr: (N, 4) uint32 array (or one 4-tuple), key: (k0, k1) -> (N, 4) uint32."""
    c = np.atleast_2d(np.asarray(ctr, dtype=np.uint64)) & MASK
    k0, k1 = np.uint64(key[0] & MASK), np.uint64(key[1] & MASK)
    for _ in range(10):
        p0 = c[:, 0] * np.uint64(M0)
        p1 = c[:, 2] * np.uint64(M1)
        hi0, lo0 = p0 >> np.uint64(32), p0 & np.uint64(MASK)
        hi1, lo1 = p1 >> np.uint64(32), p1 & np.uint64(MASK)
        c = np.stack([hi1 ^ c[:, 1] ^ k0, lo1, hi0 ^ c[:, 3] ^ k1, lo0], axis=1)
        k0 = (k0 + np.uint64(W0)) & np.uint64(MASK)
        k1 = (k1 + np.uint64(W1)) & np.uint64(MASK)
    return c.astype(np.uint32)


def gumbel(seed, b, j, step, ncols):
    """fp32 Gumbel noise of columns 0..ncols-1 of sample j of caption b at `step`."""
    seed &= (1 << 64) - 1
    quads = np.arange((ncols + 3) // 4, dtype=np.uint64)
    ctr = np.stack([quads, np.full_like(quads, step), np.full_like(quads, j), np.full_like(quads, b)], axis=1)
    x = philox4x32_10(ctr, (seed & MASK, seed >> 32)).reshape(-1)[:ncols]
    u = ((x >> 8).astype(np.float32) + np.float32(0.5)) * np.float32(2.0 ** -24)
    u = np.minimum(u, np.float32(1.0 - 2.0 ** -24))
    return -np.log(-np.log(u))


def kept_set(s, T, top_k, top_p):
    """Boolean kept mask over the raw scores s (fp32 vector) and the per-token strictly-greater mass ratio G / W (for
    boundary excuses; 0 where top-p is off)."""
    s = np.asarray(s, dtype=np.float32)
    keep = np.ones(s.shape, dtype=bool)
    if 0 < top_k < s.size:
        thr = np.sort(s)[::-1][top_k - 1]
        keep &= s >= thr
    ratio = np.zeros(s.shape)
    if top_p < 1:
        z = s / np.float32(T)
        w = np.where(keep, np.exp((z - z.max()).astype(np.float64)), 0.0)
        W = w.sum()
        order = np.argsort(-z, kind="stable")
        zs, ws = z[order], w[order]
        # mass strictly above each token: cumulative mass of the tokens with a larger z
        uniq, first = np.unique(-zs, return_index=True)
        csum = np.concatenate([[0.0], np.cumsum(ws)])
        above_sorted = csum[first[np.searchsorted(uniq, -zs)]]
        above = np.empty_like(above_sorted)
        above[order] = above_sorted
        ratio = above / W - top_p
        keep &= above < top_p * W
    return keep, ratio


def draw(s, T, top_k, top_p, g):
    """(token, kept mask, sorted perturbed values of the kept set, ratio) of one row."""
    s = np.asarray(s, dtype=np.float32)
    keep, ratio = kept_set(s, T, top_k, top_p)
    v = np.where(keep, s / np.float32(T) + g, -np.inf).astype(np.float32)
    tok = int(np.argmax(v))             # first maximum: ties to the smaller column
    return tok, keep, np.sort(v[keep])[::-1], ratio
