"""Writes tests/golden/geo_metric_cases.npz and geo_metric_data.npz.

    python tests/golden/make_geo_metric_fixtures.py <checkout of the reference>/geo-aware

The script builds synthetic captions, entity features and names, runs the reference's own JSGeoMetric over them (it is
imported from the checkout given on the command line; its data/*.pkl are read from there) and records what that class
computed: the lists it collected turned into counts per bin, the occurrence counts, the probabilities compute_metrics
derived and the Jensen-Shannon distances it printed.  geo_metric_data.npz holds the data the class was run with: the bin
edges, the number of OSM types and the train set's probabilities.  Nothing of this project is imported: the fixture is
the reference's word alone.

Two word maps: "of" has north_of .. west_of (and a plain "north" that is then an ordinary word), "plain" has north ..
west only.  The captions are written once, as words, and encoded with each map.

The hand-built rows at the end each exercise one rule; the reference is run on every one of them alone and must count
what the table says, so the recorded result is known to cover each window form and each skip path.
"""
import contextlib
import io
import os
import pickle
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
TERMS = ("near", "along", "across", "in", "north", "south", "east", "west")
FEATS = ("distance", "azimuth", "type")
T, K, C, B_RANDOM, N_RANDOM = 30, 20, 6, 40, 400
DUMMY = 124


def word_maps():
    common = ["<pad>", "<start>", "<end>", "<unk>", "the", "a", "of", "and", "is", "seen", "view", "church", "."]
    geo = ["near", "in", "across", "along"]
    az = ["north", "south", "east", "west"]
    of = common + geo + [w + "_of" for w in az] + ["north"]          # "north" is an ordinary word here
    plain = ["<pad>", "<start>", "<end>", "<unk>"] + az + geo + common[4:]
    return {"of": of, "plain": plain}


def encode(spec, words, V):
    """spec: words, "AZ:north" (the map's azimuth trigger of that term) and ("P", k) pointers."""
    wm = {w: i for i, w in enumerate(words)}
    out = []
    for s in spec:
        if isinstance(s, tuple):
            out.append(V + s[1])
        elif s.startswith("AZ:"):
            out.append(wm[s[3:] + "_of"] if "north_of" in wm else wm[s[3:]])
        else:
            out.append(wm[s])
    out = out[:T]
    return out + [wm["<pad>"]] * (T - len(out))


def name_row(idx, text, length=None, pad=DUMMY):
    codes = [ord(c) for c in text][:50]
    return [idx, len(text) if length is None else length] + codes + [pad] * (50 - len(codes))


def random_world(rng):
    ent = np.zeros((B_RANDOM + 1, K, C), np.float32)
    names = np.zeros((B_RANDOM + 1, K, 52), np.int64)
    edge_d = [0.0, 0.1, 0.5, 1.0, 2.0, 1e10, -0.5, float("nan")]
    edge_a = [-180.0, 180.0, 200.0, 250.0, -200.0, 0.0, -20.0]
    edge_t = [3.5, 986.0, -1.0, 1000.0, 985.0, 0.0, 0.25]
    for b in range(B_RANDOM):
        for k in range(K):
            ent[b, k, 0] = rng.rand()
            ent[b, k, 1] = edge_d[rng.randint(len(edge_d))] if rng.rand() < 0.1 else rng.uniform(0, 2.5)
            ent[b, k, 2] = edge_a[rng.randint(len(edge_a))] if rng.rand() < 0.1 else rng.uniform(-180, 200)
            ent[b, k, 3] = rng.rand()
            ent[b, k, 4] = edge_t[rng.randint(len(edge_t))] if rng.rand() < 0.1 else rng.randint(0, 986)
            ent[b, k, 5] = rng.rand()
            if rng.rand() < 0.15:
                names[b, k] = name_row(k, "<unk_ent>")
            else:
                n = rng.randint(3, 31)
                names[b, k] = name_row(k, "".join(chr(c) for c in rng.randint(97, 123, n)))
    return ent, names


def special_image(ent, names):
    """The last image: one slot per name rule.  Returns {label: slot}."""
    b = B_RANDOM
    rows = [("plain", "alpha", None), ("unk", "<unk_ent>", None), ("cut", "abcunk_ent", 6),
            ("unk50", "x" * 43 + "unk_ent", 50), ("full50", "y" * 50, 50), ("neglen", "x" * 43 + "unk_ent", -1),
            ("almost50", "z" * 44 + "unk_en", 50), ("len60", "w" * 43 + "unk_ent", 60), ("outside", "beta", None),
            ("restart", "ununk_ent", None), ("restart2", "unk_unk_ent", None), ("cut6", "unk_entx", 6),
            ("empty", "unk_ent", 0), ("padcut", "ab", 50)]
    slots = {}
    for k in range(K):
        label, text, length = rows[k] if k < len(rows) else ("plain%d" % k, "gamma%d" % k, None)
        names[b, k] = name_row(k, text, length)
        ent[b, k] = [0.5, 0.55, 10.0, 0.5, 5.0, 0.5]
        slots[label] = k
    ent[b, slots["outside"]] = [0.5, -1.0, 250.0, 0.5, 3.5, 0.5]
    return slots


def random_captions(rng):
    fill = ["and", "is", "seen", "view", "church", ".", "the", "a", "of"]
    links = [[], ["the"], ["a"], ["of"], ["of", "the"], ["of", "a"], ["and"], ["the", "of"], ["of", "of"], ["the", "the"]]
    link_p = np.array([5, 3, 3, 2, 3, 3, 1, 1, 1, 1], float)
    link_p /= link_p.sum()
    specs = []
    for _ in range(N_RANDOM):
        spec = ["<start>"] if rng.rand() < 0.8 else []
        for _ in range(rng.randint(1, 4)):
            spec += [fill[rng.randint(len(fill))] for _ in range(rng.randint(0, 3))]
            term = TERMS[rng.randint(8)]
            if term in TERMS[4:]:
                # sometimes the literal word "north": a trigger in the plain map, an ordinary word in the other
                spec.append("north" if term == "north" and rng.rand() < 0.3 else "AZ:" + term)
            elif rng.rand() < 0.9:
                spec.append(term)
            spec += links[rng.choice(len(links), p=link_p)]
            spec.append(("P", rng.randint(0, K + 2)))
            if rng.rand() < 0.15:
                spec.append(("P", rng.randint(0, K)))
        spec += [".", "<end>"]
        specs.append(spec)
    return specs


def special_captions(s):
    """(spec, occurrences the reference must count) for the last image; s = its slots."""
    p = ("P", s["plain"])
    return [
        (["near", p], 1),                                       # trigger at position 0, bare window at i = 1
        (["<start>", "in", "the", p], 1),                       # trigger at 1, second window
        (["AZ:north", "the", p], 1),                            # trigger at 0, second window at i = 2
        (["AZ:south", "of", "the", p], 1),                      # trigger at 0, third window at i = 3
        (["<start>", "view", "AZ:east", "of", "a", p], 1),      # trigger at 2 ... third window
        (["<start>", "and", "AZ:west", "of", p], 1),            # second window through "of"
        (["<start>", "along", "a", p], 1),
        (["<start>", "across", p, p], 1),                       # the second pointer follows a pointer
        ([p, "near", p], 1),                                    # a pointer at position 0 never counts
        (["<start>", "near", ("P", K)], 0),                     # k >= K
        (["<start>", "near", ("P", K + 1)], 0),
        (["<start>", "near", ("P", s["unk"])], 0),              # the name is <unk_ent>
        (["<start>", "near", ("P", s["cut"])], 1),              # unk_ent cut off by the length field
        (["<start>", "near", ("P", s["cut6"])], 1),
        (["<start>", "near", ("P", s["empty"])], 1),            # length 0: the empty name
        (["<start>", "near", ("P", s["unk50"])], 0),            # 50 chars ending in unk_ent
        (["<start>", "near", ("P", s["full50"])], 1),           # a 50-char name
        (["<start>", "near", ("P", s["neglen"])], 0),           # negative length: all 50 chars
        (["<start>", "near", ("P", s["len60"])], 0),            # length past 50: all 50 chars
        (["<start>", "near", ("P", s["almost50"])], 1),         # the pattern would need a 51st char
        (["<start>", "near", ("P", s["padcut"])], 1),           # length past the text: padding chars join the name
        (["<start>", "near", ("P", s["restart"])], 0),          # "ununk_ent": the search restarts on the second u
        (["<start>", "near", ("P", s["restart2"])], 0),
        (["<start>", "in", ("P", s["outside"])], 1),            # distance outside every bin, non-integer type
        (["<start>", "AZ:north", ("P", s["outside"])], 1),      # azimuth outside every bin
        (["<start>", "of", "the", p], 0),                       # no trigger
        (["<start>", "near", "and", p], 0),                     # a word that is no link
        (["near", "of", "of", p], 0),                           # of of
        (["<start>", "near", "the", "of", p], 0),               # the of
        (["<start>", "near", "the", "the", p], 0),
        (["of", "the", p], 0),                                  # third window cut off at the row's start
        (["the", p], 0),
        (["<start>", "near", "of", "the", p, "in", "a", p, "AZ:west", p], 3),
        (["<start>", "view", "."], 0),                          # no pointer at all
        ([p, p, p, p], 0),                                      # only pointers
    ]


def collect(metric_dict, nd, na, nt):
    n = np.array([metric_dict[t]["n_occurrences"] for t in TERMS], np.int64)
    size = {"distance": nd, "azimuth": na, "type": nt}
    counts = {f: np.zeros((8, size[f]), np.int64) for f in FEATS}
    lens = np.full((8, 3), -1, np.int64)
    for q, t in enumerate(TERMS):
        for j, f in enumerate(FEATS):
            if f in metric_dict[t]:
                lst = metric_dict[t][f]
                lens[q, j] = len(lst)
                counts[f][q] = [lst.count(i) for i in range(size[f])]
    return n, counts, lens


def parse_printed(text):
    js = np.full((8, 3), np.nan)
    q = None
    for line in text.splitlines():
        line = line.strip()
        if line.lower() in TERMS and line.isupper():
            q = TERMS.index(line.lower())
        elif ":" in line and q is not None and line.split(":")[0] in FEATS:
            js[q, FEATS.index(line.split(":")[0])] = float(line.split(":")[1])
    return js


def main(ref_dir):
    ref_dir = os.path.abspath(ref_dir)
    sys.path.insert(0, ref_dir)
    os.chdir(ref_dir)                       # the class opens data/*.pkl relative to the working directory
    import jensen_shannon_metric as js

    def load(name):
        with open(os.path.join(ref_dir, "data", name), "rb") as f:
            return pickle.load(f)
    bins_d, bins_a = load("bins_distance.pkl"), load("bins_azimuth.pkl")
    n_types, train = len(load("OSM_types_index.pkl")), load("geo_probability_distr_train.pkl")
    nd, na = len(bins_d), len(bins_a)
    data = {"bins_distance": np.array(bins_d, np.float64), "bins_azimuth": np.array(bins_a, np.float64),
            "n_types": np.int64(n_types)}
    for t in TERMS:
        for f in FEATS:
            if f + "_probs" in train[t]:
                data["train_%s_%s_probs" % (t, f)] = np.array(train[t][f + "_probs"], np.float64)
    np.savez_compressed(os.path.join(HERE, "geo_metric_data.npz"), **data)

    rng = np.random.RandomState(20240607)
    ent, names = random_world(rng)
    slots = special_image(ent, names)
    specs = random_captions(rng)
    image_index = list(rng.randint(0, B_RANDOM, len(specs)))
    specials = special_captions(slots)
    special_rows = np.arange(len(specs), len(specs) + len(specials))
    specs += [s for s, _ in specials]
    image_index += [B_RANDOM] * len(specials)
    image_index = np.array(image_index, np.int64)
    ent_t, names_t = torch.from_numpy(ent), torch.from_numpy(names)

    out = {"image_index": image_index, "entities": ent, "names": names, "special_rows": special_rows,
           "special_expected": np.array([e for _, e in specials], np.int64)}
    for variant, words in word_maps().items():
        wm = {w: i for i, w in enumerate(words)}
        V = len(wm)
        tokens = np.array([encode(s, words, V) for s in specs], np.int64)
        # every hand-built row alone: the reference counts what the table says
        for r, (spec, expect) in zip(special_rows, specials):
            m = js.JSGeoMetric(word_map=wm, print_metrics=False)
            m.run(tokens[r].tolist(), ent_t[image_index[r]], names_t[image_index[r]])
            got = sum(m.geo_probability_distr_generated[t]["n_occurrences"] for t in TERMS)
            assert got == expect, (variant, spec, got, expect)
        m = js.JSGeoMetric(word_map=wm, print_metrics=True)
        for r in range(len(specs)):
            m.run(tokens[r].tolist(), ent_t[image_index[r]], names_t[image_index[r]])
        gen = m.geo_probability_distr_generated
        n, counts, lens = collect(gen, nd, na, n_types)
        assert (n >= 20).all(), (variant, n)
        # a feature outside every bin and a non-integer type did occur: the lists are shorter than the occurrences,
        # or hold values that no bin counts
        assert (lens[:4, 0] < n[:4]).any() and (lens[4:, 1] < n[4:]).any(), (variant, lens, n)
        assert (counts["type"][1:4].sum(axis=1) < lens[1:4, 2]).any(), variant
        buf = io.StringIO()
        with contextlib.redirect_stdout(buf):
            m.compute_metrics(gen, m.geo_probability_distr_train)
        printed = parse_printed(buf.getvalue())
        probs = {f: np.full((8, counts[f].shape[1]), np.nan) for f in FEATS}
        for q, t in enumerate(TERMS):
            for f in FEATS:
                if f + "_probs" in gen[t]:
                    probs[f][q] = gen[t][f + "_probs"]
                    assert not np.isnan(printed[q, FEATS.index(f)]), (variant, t, f)
        out.update({"words_" + variant: np.array(words), "tokens_" + variant: tokens, "ref_n_" + variant: n,
                    "ref_len_" + variant: lens, "ref_js_" + variant: printed})
        for f in FEATS:
            out["ref_%s_%s" % (f, variant)] = counts[f]
            out["ref_probs_%s_%s" % (f, variant)] = probs[f]
        print(variant, "occurrences", n.tolist())
    np.savez_compressed(os.path.join(HERE, "geo_metric_cases.npz"), **out)
    for name in ("geo_metric_cases.npz", "geo_metric_data.npz"):
        print(name, os.path.getsize(os.path.join(HERE, name)), "bytes")


if __name__ == "__main__":
    main(sys.argv[1])
