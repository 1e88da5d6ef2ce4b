"""Plain-Python restatement of CIDEr-D on token ids (the definition in ick_amd/cider.py), written from that definition
alone.  Float64 throughout; the kernel (fp32) is held to it.

words -> n-gram counts (n = 1..4) -> tf-idf vectors with df over corpus images -> per-n clipped cosine with the
Gaussian length penalty (length = bigram count, sigma = 6) -> mean over n, mean over references, x 10."""
import math
from collections import Counter

SIGMA = 6.0


def words(row, start, end, pad, ignore=()):
    """The tokens before the first <end>, without <start>, <pad> and the ignored ids (removal closes the gap)."""
    drop = {start, pad} | set(int(i) for i in ignore)
    out = []
    for w in row:
        w = int(w)
        if w == end:
            break
        if w not in drop:
            out.append(w)
    return out


def ngrams(ws):
    """n -> Counter of n-gram tuples, n = 1..4 (term frequencies, not normalised)."""
    return {n: Counter(tuple(ws[i:i + n]) for i in range(len(ws) - n + 1)) for n in range(1, 5)}


def doc_freq(corpus, start, end, pad, ignore=()):
    """corpus: a list of images, each a list of reference rows.  Returns (df dict n-gram tuple -> number of images
    whose references together contain it, log_ref_len = log(number of images))."""
    df = Counter()
    for refs in corpus:
        seen = set()
        for r in refs:
            for c in ngrams(words(r, start, end, pad, ignore)).values():
                seen.update(c)
        df.update(seen)
    return dict(df), math.log(float(len(corpus)))


def _vec(counts, df, log_ref_len):
    vec, norm = {}, {}
    for n in range(1, 5):
        v = {g: tf * (log_ref_len - math.log(max(1.0, float(df.get(g, 0))))) for g, tf in counts[n].items()}
        vec[n] = v
        norm[n] = math.sqrt(sum(x * x for x in v.values()))
    length = sum(counts[2].values())           # coco-caption's length: the bigram count
    return vec, norm, length


def _sim(vc, nc, lc, vr, nr, lr, sigma):
    delta = float(lc - lr)
    s = []
    for n in range(1, 5):
        val = sum(min(x, vr[n].get(g, 0.0)) * vr[n].get(g, 0.0) for g, x in vc[n].items())
        if nc[n] != 0 and nr[n] != 0:
            val /= nc[n] * nr[n]
        else:
            val = 0.0
        s.append(val * math.exp(-(delta * delta) / (2.0 * sigma * sigma)))
    return s


def cider_d(cand, refs, df, log_ref_len, start, end, pad, ignore=(), sigma=SIGMA):
    """CIDEr-D of one candidate row against the reference rows of its image."""
    vc, nc, lc = _vec(ngrams(words(cand, start, end, pad, ignore)), df, log_ref_len)
    total = 0.0
    for r in refs:
        vr, nr, lr = _vec(ngrams(words(r, start, end, pad, ignore)), df, log_ref_len)
        total += sum(_sim(vc, nc, lc, vr, nr, lr, sigma)) / 4.0
    return total / len(refs) * 10.0


def cider_rows(tokens, image_index, refs, df, log_ref_len, start, end, pad, ignore=(), sigma=SIGMA):
    """Rewards of candidate rows tokens[i] against refs[image_index[i]] (refs: per image, a list of rows)."""
    return [cider_d(t, refs[int(b)], df, log_ref_len, start, end, pad, ignore, sigma)
            for t, b in zip(tokens, image_index)]


def table_to_dict(keys, counts):
    """The package's df table (keys (U, 4) uint32, 0xFFFFFFFF = unused slot; counts (U,)) as a df dict."""
    out = {}
    for k, c in zip(keys.tolist(), counts.tolist()):
        out[tuple(w for w in k if w != 0xFFFFFFFF)] = int(c)
    return out
