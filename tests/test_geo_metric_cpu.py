"""CPU-side checks of the geo-reference metric: the plain-Python restatement (tests/geo_metric_ref.py) is pinned to the
results recorded from the reference's own JSGeoMetric (tests/golden/geo_metric_cases.npz, made by
tests/golden/make_geo_metric_fixtures.py), and the package's host side -- binding, argument checks, the float64 result,
from_reference_data -- is checked without a GPU.

Tolerance of the Jensen-Shannon distances: 1e-9 absolute.  Each is the square root of a float64 sum of at most 2 x 986
terms of magnitude <= 1; the sum's rounding error is below 2e3 x 2^-53 ~ 2e-13, and the square root of a value d^2 with
that error is off by at most 2e-13 / (2 d), below 1e-9 for every d > 1e-4 (the recorded distances are all above 0.1)."""
import inspect
import os
import pickle
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import geo_metric_ref as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VARIANTS = ("of", "plain")
JS_TOL = 1e-9


@pytest.fixture(scope="module")
def fx(golden_dir):
    return R.Fixture(golden_dir)


@pytest.fixture(scope="module")
def restated(fx):
    return {v: fx.run(v) for v in VARIANTS}


def make_metric(fx, variant, **kw):
    from ick_amd.geo_metric import GeoReferenceMetric
    return GeoReferenceMetric(fx.word_map(variant), fx.bins_d, fx.bins_a, fx.n_types, fx.train, **kw)


def test_fixture_covers_the_rules(fx):
    for v in VARIANTS:
        assert (fx.cases["ref_n_" + v] >= 20).all()
    assert fx.n_types == 986 and len(fx.bins_d) == 21 and len(fx.bins_a) == 19
    # the two word maps differ in what "north" is
    assert "north_of" in fx.word_map("of") and "north_of" not in fx.word_map("plain")
    assert fx.cases["ref_n_of"][4] != fx.cases["ref_n_plain"][4]


@pytest.mark.parametrize("variant", VARIANTS)
def test_restatement_counts_equal_the_reference(fx, restated, variant):
    gen, _, marks = restated[variant]
    assert np.array_equal(gen, fx.reference_hist(variant))
    assert int((marks >= 0).sum()) == int(fx.cases["ref_n_" + variant].sum())
    # the lists the reference kept are as long as the bins counted: nothing is added when no bin matches
    lens = fx.cases["ref_len_" + variant]
    for q in range(8):
        if lens[q, 0] >= 0:
            assert gen[q, 1:65].sum() == lens[q, 0]
        if lens[q, 1] >= 0:
            assert gen[q, 65:129].sum() == lens[q, 1]


@pytest.mark.parametrize("variant", VARIANTS)
def test_restatement_hand_built_rows(fx, variant):
    rows, expect = fx.cases["special_rows"], fx.cases["special_expected"]
    for r, e in zip(rows, expect):
        gen, rnd, marks = fx.run(variant, rows=slice(int(r), int(r) + 1))
        assert gen[:, 0].sum() == e == rnd[:, 0].sum() == (marks >= 0).sum(), (int(r), int(e))


@pytest.mark.parametrize("variant", VARIANTS)
def test_restatement_js_equals_the_reference(fx, restated, variant):
    res = R.result(restated[variant][0], fx.train_probs, len(fx.bins_d), len(fx.bins_a), fx.n_types)
    ref = fx.reference_js(variant)
    for t in R.TERMS:
        assert sorted(ref[t]) == sorted(R.FEATURES[t])
        for f in R.FEATURES[t]:
            print(variant, t, f, res[t][f], ref[t][f])
            assert abs(res[t][f] - ref[t][f]) <= JS_TOL
    # and the probabilities are the reference's compute_metrics values
    gen = restated[variant][0]
    for f, n in (("distance", 21), ("azimuth", 19), ("type", 986)):
        probs = fx.cases["ref_probs_%s_%s" % (f, variant)]
        for q, t in enumerate(R.TERMS):
            if f in R.FEATURES[t]:
                assert np.array_equal(gen[q, R.COL0[f]:R.COL0[f] + n] / gen[q, 0], probs[q])


@pytest.mark.parametrize("variant", VARIANTS)
def test_result_on_host_equals_the_reference(fx, variant):
    """GeoReferenceMetric.result() is host code: fed the recorded counts it gives the recorded distances."""
    from ick_amd.geo_metric import FEATURES, TERMS, GeoReferenceCounts
    m = make_metric(fx, variant)
    h = torch.from_numpy(fx.reference_hist(variant))
    empty = torch.zeros_like(h)
    res = m.result(GeoReferenceCounts(h, empty, None))
    ref = fx.reference_js(variant)
    assert tuple(res["generated"]) == TERMS == R.TERMS and FEATURES == R.FEATURES
    for t in TERMS:
        assert res["generated"][t]["n_occurrences"] == int(fx.cases["ref_n_" + variant][TERMS.index(t)])
        for f in FEATURES[t]:
            assert abs(res["generated"][t][f] - ref[t][f]) <= JS_TOL
        assert res["random"][t] == dict({"n_occurrences": 0}, **{f: None for f in FEATURES[t]})
    total = GeoReferenceCounts(h, empty, None) + GeoReferenceCounts(h, h, None)
    assert torch.equal(total.generated, 2 * h) and torch.equal(total.random, h) and total.marks is None


def test_trigger_ids(fx):
    from ick_amd.geo_metric import trigger_ids
    for v in VARIANTS:
        wm = fx.word_map(v)
        trig, link = trigger_ids(wm)
        assert trig == R.trigger_ids(wm) and link == (wm["of"], wm["the"], wm["a"])
    trig, link = trigger_ids({"<pad>": 0, "near": 1, "north": 2})
    assert trig == [1, -1, -1, -1, 2, -1, -1, -1] and link == (-1, -1, -1)


def test_symbol_declared_exported_bound():
    import ctypes
    import ick_amd
    import ick_amd.build as build
    import ick_amd.lib as L
    hdr = open(os.path.join(ROOT, "include", "ick_amd.h")).read()
    assert re.search(r"^int\s+ick_geo_reference_counts\s*\(", hdr, flags=re.M)
    assert hasattr(ctypes.CDLL(build.build()), "ick_geo_reference_counts")
    assert len(L.SIGNATURES["ick_geo_reference_counts"]) == 26
    from ick_amd.geo_metric import GeoReferenceMetric
    assert ick_amd.GeoReferenceMetric is GeoReferenceMetric


def test_philox_lives_in_one_header():
    csrc = os.path.join(ROOT, "image-captioning-with-external-knowledge_amd", "csrc")
    owners = [f for f in sorted(os.listdir(csrc)) if f.endswith((".hip", ".h"))
              and "uint4 philox4x32_10(" in open(os.path.join(csrc, f)).read()]
    assert owners == ["philox.h"]
    for f in ("sample.hip", "geo_metric.hip"):
        assert '#include "philox.h"' in open(os.path.join(csrc, f)).read()


def test_argument_errors_before_any_launch(fx, monkeypatch):
    import ick_amd.lib as L
    import ick_amd.ops as ops
    from ick_amd.geo_metric import GeoReferenceMetric

    def no_launch():
        raise AssertionError("the library was reached")
    monkeypatch.setattr(L, "load", no_launch)
    m = make_metric(fx, "of")
    tok = torch.zeros(2, 30, dtype=torch.int64)
    idx = torch.zeros(2, dtype=torch.int32)
    ent = torch.zeros(1, 20, 6)
    names = torch.zeros(1, 20, 52, dtype=torch.int64)
    bad = [
        (tok.int(), idx, ent, names), (tok[0], idx, ent, names), (torch.zeros(2, 129, dtype=torch.int64), idx, ent, names),
        (torch.zeros(0, 30, dtype=torch.int64), idx[:0], ent, names), (tok, idx[:1], ent, names),
        (tok, idx, ent.double(), names), (tok, idx, ent[:, :, :4], names), (tok, idx, torch.zeros(1, 4096, 5), names),
        (tok, idx, ent, names.int()), (tok, idx, ent, names[:, :, :51]), (tok, idx, ent, names[:, :19]),
    ]
    for args in bad:
        with pytest.raises(L.IckError):
            m(*args)
    with pytest.raises(L.IckError):
        m(tok, idx, ent, names, row_offset=-1)
    # the op itself refuses host tensors and bad tables
    bd = torch.tensor(fx.bins_d, dtype=torch.float64)
    with pytest.raises(L.IckError):
        ops.geo_reference_counts(tok, idx, ent, names, 30, [1] * 8, 2, 3, 4, bd, bd, 986)
    # constructor
    wm = fx.word_map("of")
    for kw in (dict(n_types=0), dict(n_types=4097), dict(bins_distance=[(0, 1)] * 65), dict(bins_azimuth=[]),
               dict(train_distribution={}), dict(seed=2 ** 64), dict(seed=1.5), dict(word_map={}),
               dict(train_distribution=dict(fx.train, near={"distance_probs": [1.0]}))):
        full = dict(word_map=wm, bins_distance=fx.bins_d, bins_azimuth=fx.bins_a, n_types=fx.n_types,
                    train_distribution=fx.train)
        full.update(kw)
        with pytest.raises(L.IckError):
            GeoReferenceMetric(**full)


def test_from_reference_data(fx, tmp_path):
    from ick_amd.geo_metric import GeoReferenceMetric
    train = {t: dict({"n_occurrences": 7}, **fx.train[t]) for t in R.TERMS}
    for name, obj in (("bins_distance.pkl", fx.bins_d), ("bins_azimuth.pkl", fx.bins_a),
                      ("OSM_types_index.pkl", list(range(fx.n_types))), ("geo_probability_distr_train.pkl", train)):
        with open(tmp_path / name, "wb") as f:
            pickle.dump(obj, f)
    m = GeoReferenceMetric.from_reference_data(str(tmp_path), fx.word_map("plain"), seed=3)
    assert m.n_types == 986 and m.bins_distance == fx.bins_d and m.bins_azimuth == fx.bins_a and m.seed == 3
    assert m.train["in", "type"] == fx.train_probs["in", "type"]
    again = GeoReferenceMetric(fx.word_map("plain"), **m.constructor_data())
    assert again.train == m.train and again.seed == 3 and again.bins_distance == m.bins_distance
    with pytest.raises(FileNotFoundError):
        GeoReferenceMetric.from_reference_data(str(tmp_path / "missing"), fx.word_map("plain"))


def test_defaults_leave_evaluate_and_config_alone():
    import ick_amd.eval as E
    import ick_amd.train as T
    assert inspect.signature(E.evaluate).parameters["geo_metric"].default is None
    assert T.Config().val_geo_metric is None
