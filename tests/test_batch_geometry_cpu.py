"""Without a GPU: the batch-shape case table (tests/batch_cases.py) -- that each case's packed row count, ties,
interleaving and memory length are what its `why` claims, that the attention plans it names are the launchers'
(ops.attention_plan), that the table reaches both attention kernel families and both sides of S = 512, and that at every
case, and along every shape-change sequence, the oracle's float32 and float64 evaluations agree to a tenth of the bars the
GPU comparison uses (tests/test_batch_geometry_gpu.py), with no ReLU-flip allowance: the reference has nothing of its own
to hide behind those bars.

Float32 oracle step against the float64 one, measured on the CPU; gradients relative to max(1e-3, |ref|max), no hidden
unit set aside:

  case               scores     loss       gradient
  one_row            5.4e-07    6.8e-07    1.1e-06
  one_caption        2.0e-06    2.9e-07    1.4e-06
  one_fact           1.8e-08    2.2e-07    9.4e-07
  nearly_empty       1.3e-06    2.4e-07    7.7e-07
  equal_lengths      1.9e-06    6.6e-09    5.8e-07
  interleaved        2.5e-06    3.0e-08    8.6e-07
  rows_64            2.4e-06    1.1e-07    5.1e-07
  rows_65            2.4e-06    1.6e-07    5.8e-07
  many_short         2.5e-06    4.5e-07    6.3e-07
  long_captions      1.9e-07    2.6e-07    6.2e-07
  wide_context       2.5e-06    9.4e-07    2.2e-06
  past_matrix_core   3.7e-07    1.5e-07    1.8e-06
  base_v150          2.3e-06    9.8e-07    9.0e-07

The floors are a tenth of the GPU bars: scores 2e-5 (of max(1, |ref|max)), loss 2e-6, gradients 2e-4.

The sequences (float32 oracle with torch Adam against the float64 one, worst |loss difference| over the whole sequence):
ragged 4.8e-7 at V = 152, 6.9e-7 at V = 150 and 4.9e-7 on the projected feature maps; eviction 7.6e-7 and 6.4e-7.  The floor is a tenth of the sequence bar
2e-5.  (An eviction sequence through the table's one-row shapes strays 2.2e-6: batch_cases.EVICTION says why it has at
least 12 tokens per batch.)
"""
import pytest
import torch

import batch_cases as BC
import dropout_ref as DR
import model_cases as MC
from test_train_plan_cpu import expected

# a tenth of the GPU test's bars
SCORE_FLOOR, LOSS_FLOOR, GRAD_FLOOR, SEQ_FLOOR = DR.SCORE_BAR / 10, 2e-5 / 10, 2e-3 / 10, 2e-5 / 10

cases = pytest.mark.parametrize("c", BC.CASES, ids=lambda c: c.name)


@pytest.fixture(scope="module")
def ops():
    import ick_amd.build as build
    build.build()
    import ick_amd.ops as ops
    return ops


@pytest.fixture()
def deterministic_torch():
    # (the scatter-add behind a repeated embedding lookup otherwise sums in a changing order)
    before = torch.are_deterministic_algorithms_enabled()
    torch.use_deterministic_algorithms(True)
    yield
    torch.use_deterministic_algorithms(before)


# ------------------------------------------------------------------------------------------------ the table's premises
def test_the_issue_table_is_all_there():
    want = {"one_row": ("geo", 1, 2, 1, 0, 152), "one_caption": ("geo", 1, 9, 6, 0, 152),
            "one_fact": ("knowledge", 1, 2, 1, 1, 152), "nearly_empty": ("geo", 4, 6, 6, 0, 152),
            "equal_lengths": ("geo", 6, 9, 6, 0, 152), "interleaved": ("geo", 5, 9, 6, 0, 152),
            "rows_64": ("geo", 13, 6, 6, 0, 152), "rows_65": ("geo", 13, 6, 6, 0, 152),
            "many_short": ("geo", 64, 3, 2, 0, 152), "long_captions": ("news", 3, 52, 20, 7, 152),
            "wide_context": ("knowledge", 13, 5, 60, 40, 152), "past_matrix_core": ("knowledge", 2, 4, 200, 120, 152),
            "base_v150": ("geo", 5, 9, 6, 0, 150)}
    got = {c.name: (c.variant, c.B, c.L, c.K, c.Fn, c.V) for c in BC.CASES}
    refused = {c.name for c, _ in BC.REFUSED}
    assert {k: v for k, v in got.items() if k in want} == {k: v for k, v in want.items() if k not in refused}
    assert set(want) <= set(got) | refused
    for c in BC.CASES:
        m = c.model
        assert (m.d, m.H, m.FF_dec, m.FF_enc, m.NL, m.P) == (300, 10, 512, 512, 3, 196) and m.tier == "full"
        assert m.derived == (c.V % 8 == 0) and (c.Fn > 0) == (c.variant != "geo")


@cases
def test_batch_is_what_the_case_claims(c):
    batch, enc_out = BC.make_inputs(c)
    lens = batch["caption_lengths"].view(-1).tolist()
    assert lens == BC.case_lengths(c) and len(lens) == c.B and 1 <= min(lens) and max(lens) <= c.L
    assert tuple(batch["captions"].shape) == (c.B, c.L) and tuple(enc_out.shape) == (c.B, 300, 196)
    assert batch["entities"].shape[:2] == (c.B, c.K) and (("facts" in batch) == (c.Fn > 0))
    if c.Fn:
        assert tuple(batch["facts"].shape) == (c.B, c.Fn, 3)
    V, caps = c.V, batch["captions"]
    for b, n in enumerate(lens):       # <start> ... <end> <pad>*: what synth.make_captions writes for that length
        assert caps[b, n - 1].item() == V - 1 and not caps[b, n:].any() and (n == 1 or caps[b, 0].item() == V - 2)
        assert (caps[b, :n] > 0).all() and caps[b].max().item() < V + c.K + c.Fn
        assert not batch["caption_masks"][b, n - 1:].any()
    assert c.Mp == sum(max(0, n - 1) for n in lens) and c.S == 196 + c.K + c.Fn
    assert c.Mp >= 1


def test_premises_by_name():
    by = BC.BY_NAME
    assert by["one_row"].Mp == 1 and by["one_fact"].Mp == 1 and by["nearly_empty"].Mp == 1
    assert by["nearly_empty"].B * by["nearly_empty"].L == 24 and list(by["nearly_empty"].lengths).count(1) == 3
    assert by["one_caption"].Mp == 8 and by["one_caption"].B == 1
    assert len(set(by["equal_lengths"].lengths)) == 1 and by["equal_lengths"].B > 1          # nothing but ties
    for name in ("interleaved", "base_v150"):
        lens = list(by[name].lengths)
        rows = [n > 1 for n in lens]
        # captions with rows and captions without alternate: the valid rows are no prefix of the batch as it is given,
        # nor of the reversed batch
        assert rows != sorted(rows, reverse=True) and rows[::-1] != sorted(rows, reverse=True)
        assert lens != sorted(lens, reverse=True) and max(lens) == by[name].L and min(lens) == 1
    assert by["base_v150"].lengths == by["interleaved"].lengths and by["base_v150"].V % 8 != 0
    assert by["rows_64"].Mp == 64 and by["rows_65"].Mp == 65
    assert by["many_short"].Mp == 128 and by["many_short"].B * by["many_short"].L == 192
    assert set(BC.case_lengths(by["many_short"])) == {3} and set(BC.case_lengths(by["wide_context"])) == {5}
    lc = by["long_captions"]
    assert lc.L == 52 and BC.nqt(lc.L) == 4 and list(lc.lengths) == [52, 30, 2] and lc.L > 20
    wc = by["wide_context"]
    assert (wc.K, wc.Fn, wc.S, wc.K + wc.Fn) == (60, 40, 296, 100)
    pm = by["past_matrix_core"]
    assert pm.S == 516 and pm.K == 200
    assert {c.variant for c in BC.CASES} == {"geo", "knowledge", "news"}
    assert {1, 13, 64} <= {c.B for c in BC.CASES} and {2, 52} <= {c.L for c in BC.CASES} and {1, 200} <= {c.K for c in BC.CASES}


@cases
def test_attention_plans_are_the_launchers(ops, c):
    assert set(c.plans) == set(c.shapes)
    for name, (T, S, causal) in c.shapes.items():
        for direction, want in zip(("fwd", "bwd"), c.plans[name]):
            got = ops.attention_plan(direction, T, S, BC.DH)
            assert got is not None, (c.name, name, direction)
            assert {k: got[k] for k in expected(want)} == expected(want), (c.name, name, direction, got)
            if want[0] == "mfma":
                assert want[1] == BC.nqt(T) and want[2] == (1 if S <= 64 else 4 if S <= 256 else 5 if S <= 320 else 8)


def test_table_reaches_both_families_and_both_sides_of_512(ops):
    fam = {(name, d, p[0]) for c in BC.CASES for name, pl in c.plans.items() for d, p in zip(("fwd", "bwd"), pl)}
    for d in ("fwd", "bwd"):
        assert {("cross", d, "mfma"), ("cross", d, "general"), ("ent", d, "mfma"), ("ent", d, "general"),
                ("fact", d, "mfma"), ("fact", d, "general"), ("self_attn", d, "mfma")} <= fam
    assert any(c.S <= 512 for c in BC.CASES) and any(c.S > 512 for c in BC.CASES)
    # the general backward with dK / dV accumulated over several query chunks, inside the model
    assert any(pl[1][0] == "general" and pl[1][2] > 1 for c in BC.CASES for pl in c.plans.values())
    # S = 512 is where the matrix-core path ends for the caption lengths of the table
    assert ops.attention_plan("fwd", 4, 512, BC.DH)["mfma"] == 1 and ops.attention_plan("fwd", 4, 513, BC.DH)["mfma"] == 0
    assert {1, 4} <= {pl[0][1] for c in BC.CASES for pl in c.plans.values() if pl[0][0] == "mfma"}         # NQT
    assert {1, 4, 5} <= {pl[0][2] for c in BC.CASES for pl in c.plans.values() if pl[0][0] == "mfma"}      # MAXT


# ------------------------------------------------------------------------------------------------ the oracle's own floor
@cases
def test_float32_oracle_is_a_tenth_of_the_bars_without_relu_flip_allowance(c, deterministic_torch):
    a = BC.oracle_step(c, False)
    b = BC.oracle_step(c, True)
    want = sorted((n - 1 for n in BC.case_lengths(c)), reverse=True)
    assert a["decode_lengths"] == b["decode_lengths"] == want and sum(want) == c.Mp
    v = b["valid"]
    assert int(v.sum()) == c.Mp
    ref = b["scores"][v]
    s_err = (a["scores"].double()[v] - ref).abs().max().item() / max(1.0, ref.abs().max().item())
    l_err = abs(a["loss"] - b["loss"])
    assert a["grads"].keys() == b["grads"].keys()
    worst = (0.0, None)
    for k, gr in b["grads"].items():
        scale = max(1e-3, gr.abs().max().item())
        err = (a["grads"][k].double() - gr).abs().max().item() / scale
        if err > worst[0]:
            worst = (err, k)
    print("%-18s %.1e    %.1e    %.1e (%s)" % (c.name, s_err, l_err, worst[0], worst[1]))
    assert s_err < SCORE_FLOOR, ("scores", s_err)
    assert l_err < LOSS_FLOOR, ("loss", l_err)
    assert worst[0] < GRAD_FLOOR, ("gradient",) + worst


# (sequence, V, enc_out projected from the feature map): every oracle sequence the GPU tests compare with
SEQUENCE_RUNS = [("ragged", BC.V_DERIVED, False), ("ragged", BC.V_PLAIN, False), ("ragged", BC.V_DERIVED, True),
                 ("eviction", BC.V_DERIVED, False), ("eviction", BC.V_PLAIN, False)]


@pytest.mark.parametrize("name,V,projected", SEQUENCE_RUNS,
                         ids=["%s_v%d%s" % (n, v, "_feature_map" if p else "") for n, v, p in SEQUENCE_RUNS])
def test_float32_oracle_sequence_is_a_tenth_of_the_bar(name, V, projected, deterministic_torch):
    steps = BC.SEQUENCES[name]
    inputs = BC.sequence_inputs(steps, V, projected=projected)
    m, P = BC.sequence_model(V), BC.sequence_params(V)
    r64 = MC.oracle_loss_sequence(m, P, inputs=inputs)
    r32 = MC.oracle_loss_sequence(m, P, inputs=[(b, e.float()) for b, e in inputs], f64=False)
    errs = [abs(x - y) for x, y in zip(r32, r64)]
    print("%s V %d: float64 losses %s, float32 off by %s" % (name, V, ["%.6f" % x for x in r64], ["%.1e" % e for e in errs]))
    assert len(errs) == len(steps) == 6
    assert max(errs) < SEQ_FLOOR, errs
    # a later step on the first shape must see the updates, or a lost one would not show
    first = [i for i, s in enumerate(steps) if s[:3] == steps[0][:3]]
    assert len(first) >= 2 and abs(r64[first[-1]] - r64[0]) > 1e-3


def test_sequences_are_what_the_gpu_tests_need():
    A, tail = BC.A_SHAPE, BC.TAIL_SHAPE
    assert [s[:3] for s in BC.RAGGED] == [A, A, tail, A, A, tail] and len({s[4] for s in BC.RAGGED}) == 6
    assert BC.distinct_shapes(BC.RAGGED) == 2
    ev = [s[:3] for s in BC.EVICTION]
    assert BC.distinct_shapes(BC.EVICTION[:5]) == 5 and ev[5] == ev[0]          # one more than the four graphs kept
    bw = [s[:3] for s in BC.BITWISE]
    assert bw[:4] == [A, tail, A, A] and bw[5:] == [tail, A] and bw[4] not in (A, tail)
    assert set(BC.BITWISE[3][3]) == {1}                                         # A's shape without a single valid row
    assert len({s[:2] for s in BC.BITWISE_SS[:5]}) == 5 and BC.BITWISE_SS[5][:2] == BC.BITWISE_SS[0][:2]
    assert [s[0] for s in BC.BITWISE_CONV1] == [3, 2, 3, 2]
