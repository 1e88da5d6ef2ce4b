"""ick_geo_reference_counts / GeoReferenceMetric on the GPU: the kernel against the plain-Python restatement
(tests/geo_metric_ref.py, itself pinned to the reference in test_geo_metric_cpu.py) -- exactly, they are integers -- and
against the results recorded from the reference's own class (tests/golden/geo_metric_cases.npz).

Jensen-Shannon distances: 1e-9 absolute, as reasoned in test_geo_metric_cpu.py (float64 sums of at most 2 x 986 terms
under a square root, distances above 0.1).  The shapes are the smallest that reach every path: T around the 64-lane
passes over the row and at the limit, K around the 64-entity passes, more rows than one workgroup, both n_types."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import geo_metric_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
VARIANTS = ("of", "plain")
JS_TOL = 1e-9
WORDS = ["<pad>", "<start>", "<end>", "near", "along", "across", "in", "north_of", "south_of", "east_of", "west_of", "of",
         "the", "a", "view"]


@pytest.fixture(scope="module")
def fx(golden_dir):
    return R.Fixture(golden_dir)


@pytest.fixture(scope="module")
def restated(fx):
    return {v: fx.run(v, seed=11, row_offset=5) for v in VARIANTS}


def metric(fx, word_map, n_types=None, **kw):
    from ick_amd.geo_metric import GeoReferenceMetric
    n_types = fx.n_types if n_types is None else n_types
    train = fx.train if n_types == fx.n_types else \
        {t: {f + "_probs": ([1.0] if f == "type" else fx.train_probs[t, f]) for f in R.FEATURES[t]} for t in R.TERMS}
    return GeoReferenceMetric(word_map, fx.bins_d, fx.bins_a, n_types, train, **kw)


def launch(m, tokens, image_index, entities, names, **kw):
    c = m(torch.from_numpy(tokens).cuda(), torch.from_numpy(np.asarray(image_index)).cuda(),
          torch.from_numpy(entities).cuda(), torch.from_numpy(names).cuda(), **kw)
    return c, c.generated.cpu().numpy(), c.random.cpu().numpy(), c.marks.cpu().numpy()


def fixture_launch(fx, variant, rows=slice(None), **kw):
    m = metric(fx, fx.word_map(variant), seed=kw.pop("seed", 11))
    return (m,) + launch(m, fx.tokens(variant)[rows], fx.image_index[rows], fx.entities, fx.names, **kw)


# ------------------------------------------------------------------------------------------------ the fixture cases
@pytest.mark.parametrize("variant", VARIANTS)
def test_fixture_matches_restatement_and_reference(fx, restated, variant):
    m, c, gen, rnd, marks = fixture_launch(fx, variant, row_offset=5)
    want_gen, want_rnd, want_marks = restated[variant]
    assert np.array_equal(marks, want_marks) and np.array_equal(gen, want_gen) and np.array_equal(rnd, want_rnd)
    assert np.array_equal(gen, fx.reference_hist(variant))              # what the reference's class recorded
    res, ref = m.result(c), fx.reference_js(variant)
    for t in R.TERMS:
        assert res["generated"][t]["n_occurrences"] == int(fx.cases["ref_n_" + variant][R.TERMS.index(t)])
        for f in R.FEATURES[t]:
            print(variant, t, f, res["generated"][t][f], ref[t][f])
            assert abs(res["generated"][t][f] - ref[t][f]) <= JS_TOL
    want = R.result(want_rnd, fx.train_probs, len(fx.bins_d), len(fx.bins_a), fx.n_types)
    for t in R.TERMS:
        assert res["random"][t]["n_occurrences"] == want[t]["n_occurrences"]
        for f in R.FEATURES[t]:
            assert abs(res["random"][t][f] - want[t][f]) <= JS_TOL


def test_same_bits_on_two_runs_and_in_deterministic_mode(fx, restated):
    import ick_amd.ops as ops
    _, _, gen, rnd, marks = fixture_launch(fx, "of", row_offset=5)
    _, _, gen2, rnd2, marks2 = fixture_launch(fx, "of", row_offset=5)
    assert np.array_equal(gen, gen2) and np.array_equal(rnd, rnd2) and np.array_equal(marks, marks2)
    before = ops.is_deterministic()
    ops.set_deterministic(True)
    try:
        _, _, gen3, rnd3, marks3 = fixture_launch(fx, "of", row_offset=5)
    finally:
        ops.set_deterministic(before)
    assert np.array_equal(gen, gen3) and np.array_equal(rnd, rnd3) and np.array_equal(marks, marks3)


def test_half_batches_add_up_to_the_full_batch(fx, restated):
    m, full, gen, rnd, _ = fixture_launch(fx, "plain", row_offset=5)
    n = len(fx.image_index)
    h = n // 2
    _, a, _, _, marks_a = fixture_launch(fx, "plain", rows=slice(0, h), row_offset=5)
    _, b, _, _, marks_b = fixture_launch(fx, "plain", rows=slice(h, n), row_offset=5 + h)
    total = a + b
    assert torch.equal(total.generated, full.generated) and torch.equal(total.random, full.random)
    assert np.array_equal(np.concatenate([marks_a, marks_b]), restated["plain"][2])
    assert m.result(total) == m.result(full)


def test_random_baseline(fx, restated):
    _, _, gen, rnd, marks = fixture_launch(fx, "of", row_offset=5)
    rows, cols = np.nonzero(marks >= 0)
    assert len(rows) > 300
    drawn = (marks[rows, cols] >> 12) & 0xFFF
    for r, k in zip(rows, drawn):                                        # never an unk_ent entity
        assert not R.is_unk(fx.names[fx.image_index[r], k])
    assert np.array_equal(marks, restated["of"][2])                      # the restatement's draw
    assert np.array_equal(rnd[:, 0], gen[:, 0]) and not np.array_equal(rnd, gen)
    _, _, gen_s, rnd_s, marks_s = fixture_launch(fx, "of", row_offset=5, seed=12)
    _, _, gen_o, rnd_o, marks_o = fixture_launch(fx, "of", row_offset=6)
    for g, m2 in ((gen_s, marks_s), (gen_o, marks_o)):
        assert np.array_equal(g, gen)                                    # the generated side does not see the draw
        assert np.array_equal(m2 >= 0, marks >= 0) and np.array_equal(m2[rows, cols] & ~0xFFF000,
                                                                      marks[rows, cols] & ~0xFFF000)
        assert (((m2[rows, cols] >> 12) & 0xFFF) != drawn).mean() > 0.5  # most draws moved
    want = fx.run("of", seed=12, row_offset=5)
    assert np.array_equal(marks_s, want[2]) and np.array_equal(rnd_s, want[1])
    big = fx.run("of", seed=-3, row_offset=2 ** 32 - 7, rows=slice(0, 40))
    _, _, _, rnd_b, marks_b = fixture_launch(fx, "of", rows=slice(0, 40), seed=-3, row_offset=2 ** 32 - 7)
    assert np.array_equal(marks_b, big[2]) and np.array_equal(rnd_b, big[1])


# ------------------------------------------------------------------------------------------------ small shapes
def make_case(N, T, K, B, n_types, seed, pointers="mixed"):
    rng = np.random.RandomState(seed)
    V = len(WORDS)
    if pointers == "only":
        tokens = V + rng.randint(0, K, (N, T))
    elif pointers == "none":
        tokens = rng.randint(0, V, (N, T))
    else:
        # triggers, links and pointers each about a third: the windows are frequent; pointers reach past K
        kind = rng.rand(N, T)
        tokens = np.where(kind < 0.35, rng.randint(3, 11, (N, T)),
                          np.where(kind < 0.6, rng.randint(11, V, (N, T)), V + rng.randint(0, K + 2, (N, T))))
        tokens[rng.rand(N, T) < 0.05] = 0
    ent = rng.uniform(0, 2.5, (B, K, 5)).astype(np.float32)
    ent[:, :, 2] = rng.uniform(-200, 220, (B, K))
    ent[:, :, 4] = np.where(rng.rand(B, K) < 0.8, rng.randint(0, n_types + 1, (B, K)), rng.rand(B, K))
    names = np.full((B, K, 52), 124, np.int64)
    for b in range(B):
        for k in range(K):
            text = "<unk_ent>" if rng.rand() < 0.25 else "e%d_%d" % (b, k)
            names[b, k, 0], names[b, k, 1] = k, len(text)
            names[b, k, 2:2 + len(text)] = [ord(c) for c in text]
    idx = rng.randint(0, B, N)                       # images shared by several rows
    if N >= 4:
        idx[1], idx[N - 1] = -1, B                   # out of range on both sides
    return tokens.astype(np.int64), idx.astype(np.int64), ent, names


SHAPES = [  # N, T, K, B, n_types
    (1, 1, 1, 1, 1), (1, 2, 1, 1, 986), (3, 3, 20, 2, 986), (5, 4, 20, 2, 1), (63, 64, 64, 7, 986), (9, 65, 65, 3, 986),
    (130, 30, 20, 11, 986), (6, 128, 65, 2, 1), (7, 128, 200, 2, 986),
]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "N%d_T%d_K%d_B%d_types%d" % s)
def test_small_shapes_match_restatement(fx, shape):
    N, T, K, B, n_types = shape
    wm = {w: i for i, w in enumerate(WORDS)}
    tokens, idx, ent, names = make_case(N, T, K, B, n_types, seed=sum(shape))
    m = metric(fx, wm, n_types=n_types, seed=2 ** 63 + 5)
    _, gen, rnd, marks = launch(m, tokens, idx, ent, names, row_offset=3)
    want = R.run(tokens, idx, ent, names, wm, fx.bins_d, fx.bins_a, n_types, seed=2 ** 63 + 5, row_offset=3)
    assert marks.shape == (N, T)
    assert np.array_equal(marks, want[2]) and np.array_equal(gen, want[0]) and np.array_equal(rnd, want[1])
    if N >= 4:
        assert (marks[1] == -1).all() and (marks[N - 1] == -1).all()
    if T >= 30 and N * T >= 500:
        assert (marks >= 0).sum() > 0                # the case does count something


@pytest.mark.parametrize("words", [["near", 0], ["north_of", "the", 0], ["south_of", "of", "a", 0], ["view", 0], [0],
                                   ["of", "the", 0], ["the", 0]], ids=lambda w: "_".join(str(x) for x in w))
def test_the_shortest_rows(fx, words):
    """T = 1..4, K = 1: every window exactly where the row begins."""
    wm = {w: i for i, w in enumerate(WORDS)}
    tokens = np.array([[wm[w] if isinstance(w, str) else len(wm) + w for w in words]], np.int64)
    _, _, ent, names = make_case(1, 1, 1, 1, 986, seed=2)
    names[0, 0, 1] = 0                                                    # the empty name: not unk_ent
    _, gen, rnd, marks = launch(metric(fx, wm), tokens, [0], ent, names)
    want = R.run(tokens, [0], ent, names, wm, fx.bins_d, fx.bins_a, 986)
    assert np.array_equal(marks, want[2]) and np.array_equal(gen, want[0]) and np.array_equal(rnd, want[1])
    counted = len(words) >= 2 and words[0] in ("near", "north_of", "south_of")
    assert (marks >= 0).sum() == int(counted) and (not counted or marks[0, -1] == R.TERMS.index(
        words[0].split("_")[0]) << 24)


@pytest.mark.parametrize("pointers", ["only", "none"])
def test_rows_of_only_pointers_or_none(fx, pointers):
    wm = {w: i for i, w in enumerate(WORDS)}
    tokens, idx, ent, names = make_case(5, 30, 20, 2, 986, seed=4, pointers=pointers)
    c, gen, rnd, marks = launch(metric(fx, wm), tokens, idx, ent, names)
    assert (marks == -1).all() and not gen.any() and not rnd.any()
    res = metric(fx, wm).result(c)
    assert res["generated"]["in"] == {"n_occurrences": 0, "distance": None, "type": None}


def test_a_word_map_without_some_words(fx):
    """Only "near" and plain "north" exist: nothing else triggers, and <pad> = 0 is no stand-in for the missing ids."""
    wm = {w: i for i, w in enumerate(["<pad>", "x1", "x2", "near", "x3", "x4", "x5", "north", "x6", "x7", "x8", "x9", "x10",
                                      "x11", "x12"])}
    tokens, idx, ent, names = make_case(40, 30, 20, 3, 986, seed=9)
    _, gen, rnd, marks = launch(metric(fx, wm), tokens, idx, ent, names)
    want = R.run(tokens, idx, ent, names, wm, fx.bins_d, fx.bins_a, 986)
    assert np.array_equal(marks, want[2]) and np.array_equal(gen, want[0]) and np.array_equal(rnd, want[1])
    assert gen[0, 0] > 0 and gen[4, 0] > 0 and not gen[[1, 2, 3, 5, 6, 7], 0].any()


def test_the_library_refuses_bad_arguments(fx):
    import ick_amd.lib as L
    import ick_amd.ops as ops
    wm = {w: i for i, w in enumerate(WORDS)}
    tokens, idx, ent, names = (torch.from_numpy(x).cuda() for x in make_case(4, 8, 5, 2, 986, seed=1))
    bd = torch.tensor(fx.bins_d, dtype=torch.float64).cuda()
    ba = torch.tensor(fx.bins_a, dtype=torch.float64).cuda()
    trig = R.trigger_ids(wm)
    ok = lambda **kw: ops.geo_reference_counts(  # noqa: E731
        kw.get("tokens", tokens), idx, ent, names, kw.get("V", len(wm)), kw.get("trig", trig), wm["of"], wm["the"], wm["a"],
        bd, ba, kw.get("n_types", 986), row_offset=kw.get("row_offset", 0))
    ok()
    for kw in (dict(V=3), dict(trig=trig[:7]), dict(trig=[len(wm)] * 8), dict(n_types=4097), dict(row_offset=-1),
               dict(tokens=torch.zeros(4, 129, dtype=torch.int64).cuda())):
        with pytest.raises(L.IckError):
            ok(**kw)
    lib = L.load()
    idx32 = idx.int()
    args = [tokens.data_ptr(), 4, 8, idx32.data_ptr(), ent.data_ptr(), names.data_ptr(), 2, 5, 5, len(wm),
            (L.i32 * 8)(*trig), 1, 2, 3, bd.data_ptr(), 21, ba.data_ptr(), 19, 986, 1153, 0, 0]
    out = torch.zeros(3, 8 * 1153, dtype=torch.int32).cuda()
    tail = [out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(), None]
    bad = {2: 129, 7: 4096, 8: 4, 15: 65, 17: 0, 18: 4097, 19: 1114, 21: -1, 9: 0}
    for pos, val in bad.items():
        a = list(args)
        a[pos] = val
        assert lib.ick_geo_reference_counts(*(a + tail)) == -1, pos
    assert lib.ick_geo_reference_counts(*(args + [tail[0], tail[1], tail[1], None])) == -1
    assert lib.ick_geo_reference_counts(*(args + [None, tail[1], tail[2], None])) == -1
    torch.cuda.synchronize()
    assert not out.any().item()                                           # nothing was launched


# ------------------------------------------------------------------------------------------------ eval.py, train.py
@pytest.fixture(scope="module")
def toy(tmp_path_factory):
    """A synthetic geo data set and a decoder with synthetic parameters on it."""
    import ick_amd
    import ick_amd.synth as synth
    root = tmp_path_factory.mktemp("geo_metric")
    data_dir = str(root / "data")
    V, K = 60, 6
    wm = synth.write_dataset(data_dir, "toy", "geo", n_train=4, n_val=8, n_test=6, L=12, K=K, V=V)
    models = ick_amd.load_models("geo")
    dec = models.DecoderTransformer(wm, 300, 512, 512, 10, 3)
    dec.load_state_dict(synth.make_params("geo", V, 1), strict=False)
    enc = models.Encoder(emb_dim=300)
    cw, cb = synth.make_conv1(1)
    with torch.no_grad():
        enc.conv1.weight.copy_(cw)
        enc.conv1.bias.copy_(cb)
    return dict(root=root, data_dir=data_dir, wm=wm, dec=dec.cuda().eval(), enc=enc.cuda().eval(), K=K)


def observed_word_map(seqs, wm, K):
    """The synthetic vocabulary has no prepositions: name the words that the decoder did put in front of pointers."""
    V = len(wm)
    special = {wm["<pad>"], wm["<start>"], wm["<end>"], wm["<unk>"]}
    seen = {}
    for s in seqs:
        for i in range(1, len(s)):
            if V <= s[i] < V + K and s[i - 1] < V and s[i - 1] not in special:
                seen[s[i - 1]] = seen.get(s[i - 1], 0) + 1
    ranked = sorted(seen, key=lambda t: (-seen[t], t))
    names = ["near", "north_of", "in", "the", "along", "south_of", "of", "across", "east_of", "a", "west_of"]
    rename = dict(zip(ranked, names))
    return {rename.get(i, w): i for w, i in wm.items()}


def test_evaluate_with_geo_metric(fx, toy):
    import ick_amd.eval as ev
    from ick_amd.datasets import CaptionDataset
    from ick_amd.geo_metric import GeoReferenceMetric
    wm, dec, enc, K = toy["wm"], toy["dec"], toy["enc"], toy["K"]
    ds = CaptionDataset(toy["data_dir"], "toy", "TEST")
    loader = lambda: torch.utils.data.DataLoader(ds, batch_size=4, shuffle=False)   # noqa: E731
    csv = str(toy["root"] / "generated_captions.csv")
    sample = dict(num_samples=4, seed=5, temperature=3.0)
    caps0, seqs0 = ev.evaluate(enc, dec, loader(), wm, max_caption_len=10, out_csv=csv, sample=sample)
    plain_csv = open(csv).read()
    gwm = observed_word_map(seqs0, wm, K)
    m = GeoReferenceMetric(gwm, fx.bins_d, fx.bins_a, fx.n_types, fx.train, seed=21)
    caps, seqs, res = ev.evaluate(enc, dec, loader(), wm, max_caption_len=10, out_csv=csv, sample=sample, geo_metric=m)
    assert caps == caps0 and seqs == seqs0 and open(csv).read() == plain_csv and set(res) == {"geo_js"}
    ent = np.asarray(ds.entity_features, dtype=np.float32)
    names = np.asarray(ds.entity_names, dtype=np.int64)
    want = R.run(np.asarray(seqs), np.repeat(np.arange(6), 4), ent, names, gwm, fx.bins_d, fx.bins_a, fx.n_types, seed=21)
    assert want[0][:, 0].sum() > 0                                        # the captions do hold geo references
    for side, hist in (("generated", want[0]), ("random", want[1])):
        ref = R.result(hist, fx.train_probs, len(fx.bins_d), len(fx.bins_a), fx.n_types)
        for t in R.TERMS:
            assert res["geo_js"][side][t]["n_occurrences"] == ref[t]["n_occurrences"], (side, t)
            for f in R.FEATURES[t]:
                got = res["geo_js"][side][t][f]
                assert (got is None) == (ref[t][f] is None) and (got is None or abs(got - ref[t][f]) <= JS_TOL)
    # greedy rows, one per image, beside the caption metrics
    from ick_amd.metrics import CaptionMetrics
    refs_of = lambda bi, batch: batch[1].unsqueeze(1)                    # noqa: E731
    cm = CaptionMetrics(wm, pointer_base=len(wm))
    _, seqs_g, res_m = ev.evaluate(enc, dec, loader(), wm, max_caption_len=10, out_csv=csv, metrics=cm, refs=refs_of)
    _, seqs_g2, res_g = ev.evaluate(enc, dec, loader(), wm, max_caption_len=10, out_csv=csv, metrics=cm, refs=refs_of,
                                    geo_metric=m)
    assert seqs_g2 == seqs_g and {k: v for k, v in res_g.items() if k != "geo_js"} == res_m
    want_g = R.run(np.asarray(seqs_g), np.arange(6), ent, names, gwm, fx.bins_d, fx.bins_a, fx.n_types, seed=21)
    assert [res_g["geo_js"]["generated"][t]["n_occurrences"] for t in R.TERMS] == want_g[0][:, 0].tolist()
    # without the argument: what it returned before
    assert len(ev.evaluate(enc, dec, loader(), wm, max_caption_len=10, out_csv=csv)) == 2


def test_validate_with_geo_metric(fx, toy, capsys):
    import ick_amd.train as tr
    from ick_amd.datasets import CaptionDataset
    from ick_amd.geo_metric import GeoReferenceMetric
    wm, dec, enc, K = toy["wm"], toy["dec"], toy["enc"], toy["K"]
    ds = CaptionDataset(toy["data_dir"], "toy", "VAL")
    batches = lambda: torch.utils.data.DataLoader(ds, batch_size=4, shuffle=False)  # noqa: E731
    seqs = []
    with torch.no_grad():
        for batch in batches():
            seqs += dec.predict(enc(batch[0].cuda().float()), 12, batch[4]).t().cpu().tolist()
    gwm = observed_word_map(seqs, wm, K)
    data = GeoReferenceMetric(gwm, fx.bins_d, fx.bins_a, fx.n_types, fx.train, seed=4).constructor_data()
    base = dict(variant="geo", data_dir=toy["data_dir"], data_name="toy", batch_size=4, workers=0)
    crit = tr.make_criteria(wm["<pad>"])[1].cuda()
    dev = torch.device("cuda", torch.cuda.current_device())
    loss0, res0 = tr.validate(batches(), enc, dec, crit, tr.Config(val_caption_metrics=True, **base), dev)
    assert "geo_js" not in res0
    old = dec.word_map
    dec.word_map = gwm                                                   # same ids; the metric reads the decoder's map
    try:
        loss1, res1 = tr.validate(batches(), enc, dec, crit,
                                  tr.Config(val_caption_metrics=True, val_geo_metric=data, **base), dev)
    finally:
        dec.word_map = old
    assert abs(loss1 - loss0) < 1e-6 and {k: v for k, v in res1.items() if k != "geo_js"} == res0
    assert "geo references, generated" in capsys.readouterr().out
    want = R.run(np.asarray(seqs), np.arange(8), np.asarray(ds.entity_features, dtype=np.float32),
                 np.asarray(ds.entity_names, dtype=np.int64), gwm, fx.bins_d, fx.bins_a, fx.n_types, seed=4)
    for side, hist in (("generated", want[0]), ("random", want[1])):
        assert [res1["geo_js"][side][t]["n_occurrences"] for t in R.TERMS] == hist[:, 0].tolist()
    with pytest.raises(ValueError):
        tr.main(tr.Config(val_geo_metric=data, epochs=0, **base))
