"""Plain-Python restatement of the geo-reference counts and their Jensen-Shannon distances (the definition in
ick_amd/geo_metric.py), written from that definition alone: lists of ints, one loop per caption, math.log2.  The kernel
is held to it, and it is held to results recorded from the reference's own class (tests/golden/geo_metric_cases.npz).

run() returns the two histograms in the kernel's layout -- (8, 1 + 64 + 64 + n_types padded to 64), column 0 =
n_occurrences -- and the (N, T) marks, so a comparison is one array_equal."""
import math

import numpy as np

from sample_ref import philox4x32_10

TERMS = ("near", "along", "across", "in", "north", "south", "east", "west")
FEATURES = {"near": ("distance",), "along": ("distance", "type"), "across": ("distance", "type"),
            "in": ("distance", "type"), "north": ("azimuth",), "south": ("azimuth",), "east": ("azimuth",),
            "west": ("azimuth",)}
UNK = [ord(c) for c in "unk_ent"]
MAX_BINS, CHARS = 64, 50
COL0 = {"distance": 1, "azimuth": 1 + MAX_BINS, "type": 1 + 2 * MAX_BINS}


def width(n_types):
    return 1 + 2 * MAX_BINS + (n_types + 63) // 64 * 64


def trigger_ids(word_map):
    az = ["north", "south", "east", "west"]
    if "north_of" in word_map:
        az = [w + "_of" for w in az]
    return [word_map.get(w, -1) for w in ["near", "along", "across", "in"] + az]


def effective_name(row):
    """row = [idx, length, 50 chars]: the character codes the name stands for."""
    length, chars = int(row[1]), [int(c) for c in row[2:2 + CHARS]]
    return chars if length < 0 else chars[:length]


def is_unk(row):
    name = effective_name(row)
    return any(name[s:s + 7] == UNK for s in range(len(name) - 6))


def find_bin(bins, x):
    x = float(x)
    for b, (lo, hi) in enumerate(bins):
        if lo <= x < hi:
            return b
    return None


def term_of(tokens, i, V, trig, of, the, a):
    """The term (0..7) of the window in front of position i, or None."""
    def trigger(t):
        return trig.index(t) if 0 <= t < V and t in trig else None

    def one_of(t, ids):
        return t >= 0 and t in [x for x in ids if x >= 0]
    p0 = tokens[i - 1]
    if p0 >= V:
        return None
    if trigger(p0) is not None:
        return trigger(p0)
    if i >= 2 and trigger(tokens[i - 2]) is not None and one_of(p0, (of, the, a)):
        return trigger(tokens[i - 2])
    if i >= 3 and trigger(tokens[i - 3]) is not None and one_of(tokens[i - 2], (of,)) and one_of(p0, (the, a)):
        return trigger(tokens[i - 3])
    return None


def add(hist, term, feats, bins_d, bins_a, n_types):
    hist[term, 0] += 1
    if term < 4:
        b = find_bin(bins_d, feats[1])
        if b is not None:
            hist[term, COL0["distance"] + b] += 1
    else:
        b = find_bin(bins_a, feats[2])
        if b is not None:
            hist[term, COL0["azimuth"] + b] += 1
    if 1 <= term <= 3:
        x = float(feats[4])
        if math.isfinite(x) and x == math.floor(x) and 0 <= x < n_types:
            hist[term, COL0["type"] + int(x)] += 1


def run(tokens, image_index, entities, names, word_map, bins_d, bins_a, n_types, seed=0, row_offset=0):
    """-> (generated, random, marks) numpy int32 arrays."""
    tokens, entities, names = np.asarray(tokens), np.asarray(entities), np.asarray(names)
    N, T = tokens.shape
    B, K = entities.shape[:2]
    V = len(word_map)
    trig = trigger_ids(word_map)
    of, the, a = (word_map.get(w, -1) for w in ("of", "the", "a"))
    gen = np.zeros((8, width(n_types)), np.int32)
    rnd = np.zeros_like(gen)
    marks = np.full((N, T), -1, np.int32)
    seed &= (1 << 64) - 1
    key = (seed & 0xFFFFFFFF, seed >> 32)
    for n in range(N):
        img = int(image_index[n])
        if not 0 <= img < B:
            continue
        row = [int(t) for t in tokens[n]]
        known = None
        for i in range(1, T):
            k = row[i] - V
            if k < 0 or k >= K:
                continue
            term = term_of(row, i, V, trig, of, the, a)
            if term is None or is_unk(names[img, k]):
                continue
            if known is None:
                known = [s for s in range(K) if not is_unk(names[img, s])]
            r = row_offset + n
            x = int(philox4x32_10((i, r & 0xFFFFFFFF, r >> 32, 0), key)[0, 0])
            rk = known[x % len(known)]
            add(gen, term, entities[img, k], bins_d, bins_a, n_types)
            add(rnd, term, entities[img, rk], bins_d, bins_a, n_types)
            marks[n, i] = term << 24 | rk << 12 | k
    return gen, rnd, marks


def js_distance(p, q):
    def kl(a, b):
        return sum(x * math.log2(x / y) for x, y in zip(a, b) if x != 0 and y != 0)
    m = [0.5 * (x + y) for x, y in zip(p, q)]
    return math.sqrt(0.5 * kl(p, m) + 0.5 * kl(q, m))


def result(hist, train_probs, n_dist, n_az, n_types):
    """{term: {"n_occurrences", feature: JS distance or None}}; train_probs[term, feature] = the train set's probs."""
    size = {"distance": n_dist, "azimuth": n_az, "type": n_types}
    out = {}
    for q, term in enumerate(TERMS):
        n = int(hist[q, 0])
        out[term] = {"n_occurrences": n}
        for f in FEATURES[term]:
            counts = hist[q, COL0[f]:COL0[f] + size[f]]
            out[term][f] = js_distance(list(train_probs[term, f]), [int(c) / n for c in counts]) if n else None
    return out


class Fixture:
    """tests/golden/geo_metric_cases.npz + geo_metric_data.npz (made by tests/golden/make_geo_metric_fixtures.py from
    the reference's own class), as plain Python / numpy data."""

    def __init__(self, golden_dir):
        import os
        self.cases = np.load(os.path.join(golden_dir, "geo_metric_cases.npz"))
        data = np.load(os.path.join(golden_dir, "geo_metric_data.npz"))
        self.bins_d = [tuple(r) for r in data["bins_distance"].tolist()]
        self.bins_a = [tuple(r) for r in data["bins_azimuth"].tolist()]
        self.n_types = int(data["n_types"])
        self.train_probs = {(t, f): data["train_%s_%s_probs" % (t, f)].tolist() for t in TERMS for f in FEATURES[t]}
        self.train = {t: {f + "_probs": self.train_probs[t, f] for f in FEATURES[t]} for t in TERMS}
        self.image_index, self.entities, self.names = (self.cases[k] for k in ("image_index", "entities", "names"))

    def word_map(self, variant):
        return {str(w): i for i, w in enumerate(self.cases["words_" + variant])}

    def tokens(self, variant):
        return self.cases["tokens_" + variant]

    def reference_hist(self, variant):
        """The reference's recorded counts in the kernel's histogram layout."""
        h = np.zeros((8, width(self.n_types)), np.int32)
        h[:, 0] = self.cases["ref_n_" + variant]
        for f in ("distance", "azimuth", "type"):
            c = self.cases["ref_%s_%s" % (f, variant)]
            h[:, COL0[f]:COL0[f] + c.shape[1]] = c
        return h

    def reference_js(self, variant):
        """{term: {feature: the JS distance the reference printed}}"""
        js = self.cases["ref_js_" + variant]
        return {t: {f: float(js[q, ("distance", "azimuth", "type").index(f)]) for f in FEATURES[t]}
                for q, t in enumerate(TERMS)}

    def run(self, variant, seed=0, row_offset=0, rows=None):
        rows = slice(None) if rows is None else rows
        return run(self.tokens(variant)[rows], self.image_index[rows], self.entities, self.names,
                   self.word_map(variant), self.bins_d, self.bins_a, self.n_types, seed, row_offset)
