"""The device caption metrics (ick_caption_metrics, ick_caption_metric_sums, ick_amd.CaptionMetrics) on the GPU: the
kernel against the plain-Python restatement (metrics_ref.py) in general and SCST-layout mode, limits and bad indices,
the totals and the corpus result, SelfCriticalStep with a mixed MetricReward against a twin whose host reward_fn is the
restatement, and the training / evaluation scripts' use of the metrics.

Tolerances.  counts and pointers are integers and must be equal.  bleu and rouge_l are held to the float64 restatement
within a relative 1e-5, with an absolute floor of 1e-12 for the exact zeros.  result() is held to the restatement's
corpus result within 1e-9: BLEU and the pointer ratios come from integer sums; ROUGE_L is the mean of the rows' float32
values, so there the restatement's per-caption value is rounded to float32 first, as the rows hold it (against the
unrounded float64 mean it is held to float32's half-ulp, 6e-8)."""
import math
import os

import numpy as np
import pytest
import torch

import ick_amd.ops as ops
import ick_amd.synth as synth
import metrics_ref as R
from cider_ref import cider_rows, table_to_dict
from ick_amd.cider import CiderD
from ick_amd.lib import IckError
from ick_amd.metrics import CaptionMetrics, MetricReward
from test_cider_gpu import _refs_for, _twin

pytestmark = pytest.mark.gpu

V = 1004                                     # words 1..1000, <unk>, <start>, <end>; pointer ids are >= V
WM = synth.make_word_map(V)
START, END, PAD = WM["<start>"], WM["<end>"], WM["<pad>"]
SMALL = np.arange(1, 5)                      # a 4-id alphabet: many repeats, long LCS, clipping that bites
BIG = np.arange(1, 1001)
IGNORE16 = tuple(range(5, 21))


def _close(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    err = np.abs(got - want)
    assert (err <= np.maximum(1e-5 * np.abs(want), 1e-12)).all(), (err.max(), got[err.argmax()], want[err.argmax()])


def _rows(rng, n_rows, L, ids, pointers, ignore):
    """Rows of every kind in turn: <end> somewhere / first / last / absent, only <pad>, and one with <start>, <pad>
    gaps and ignored ids inside."""
    out = []
    for i in range(n_rows):
        w = rng.choice(ids, size=L)
        if pointers:
            w = np.where(rng.random(L) < 0.3, V + rng.integers(0, 6, size=L), w)
        if ignore:
            w = np.where(rng.random(L) < 0.1, rng.choice(ignore, size=L), w)
        kind = i % 6
        if kind == 0:
            e = int(rng.integers(0, L))
            w[e] = END
            w[e + 1:] = PAD
        elif kind == 1:
            w[0] = END
        elif kind == 2:
            w[L - 1] = END
        elif kind == 4:
            w[:] = PAD
        elif kind == 5:
            w[0] = START
            w[rng.random(L) < 0.2] = PAD
        out.append(w)                        # kind 3: no <end>
    return np.array(out, dtype=np.int64)


def _problem(T, Lr, M, N, ids, pointers, ignore, seed, B=None):
    rng = np.random.default_rng(seed)
    B = B or min(N, 5)
    refs = _rows(rng, B * M, Lr, ids, pointers, ignore).reshape(B, M, Lr)
    cands = _rows(rng, N, T, ids, pointers, ignore)
    if N >= 7 and T == Lr:
        cands[6] = refs[6 % B, 0]            # a candidate that is one of its references
    img = (np.arange(N) % B).astype(np.int64)
    return cands, img, refs


def _restate(cands, img, refs, ignore=(), pointer_base=V):
    return R.caption_rows(cands, img, [list(r) for r in refs], START, END, PAD, ignore, pointer_base)


def _check_rows(got, want):
    counts, bleu, rouge, ptrs = (t.cpu().numpy() for t in got[:4])
    assert np.array_equal(counts, np.array([w.counts for w in want], dtype=np.int32))
    assert np.array_equal(ptrs, np.array([w.pointers for w in want], dtype=np.int32))
    _close(bleu, [w.bleu for w in want])
    _close(rouge, [w.rouge_l for w in want])


# ------------------------------------------------------------------------------------------------ kernel vs restatement
CASES = [  # T, Lr, M, N, alphabet, pointers, ignore
    (1, 1, 1, 1, SMALL, False, ()),
    (2, 20, 2, 7, SMALL, False, ()),
    (3, 64, 5, 7, BIG, True, ()),
    (4, 20, 16, 7, SMALL, True, IGNORE16),
    (5, 1, 2, 130, SMALL, False, ()),
    (63, 64, 5, 7, SMALL, False, IGNORE16),
    (64, 64, 16, 7, SMALL, True, ()),
    (64, 20, 1, 130, BIG, True, IGNORE16),
    (20, 20, 5, 130, SMALL, True, ()),
]


@pytest.mark.parametrize("case", range(len(CASES)))
def test_general_mode_matches_restatement(case):
    T, Lr, M, N, ids, pointers, ignore = CASES[case]
    cands, img, refs = _problem(T, Lr, M, N, ids, pointers, ignore, seed=case)
    m = CaptionMetrics(WM, ignore=ignore, pointer_base=V)
    t, i, r = torch.from_numpy(cands).cuda(), torch.from_numpy(img).cuda(), torch.from_numpy(refs).cuda()
    got = m(t, i, r)
    want = _restate(cands, img, refs, ignore)
    _check_rows(got, want)
    again = m(t, i, r)
    assert all(torch.equal(a, b) for a, b in zip(got, again))                 # bit-identical
    off = CaptionMetrics(WM, ignore=ignore)(t, i, r)                          # no pointer base: zero pointer counts
    assert not off.pointers.any() and torch.equal(off.counts, got.counts) and torch.equal(off.bleu, got.bleu)
    if N >= 7 and ids is SMALL and Lr >= 20:                                  # both ends of the range were exercised
        assert max(w.bleu[0] for w in want) > 0.5 and min(w.bleu[0] for w in want) < 1e-6


def test_two_dimensional_refs_and_beta():
    cands, img, refs = _problem(12, 12, 1, 7, SMALL, False, (), seed=40)
    t, i = torch.from_numpy(cands).cuda(), torch.from_numpy(img).cuda()
    m = CaptionMetrics(WM, beta=2.0)
    got = m(t, i, torch.from_numpy(refs[:, 0]).cuda())                        # (B, L) references
    want = R.caption_rows(cands, img, [list(r) for r in refs], START, END, PAD, (), None, beta=2.0)
    _check_rows(got, want)


def test_limits_and_bad_indices():
    cands, img, refs = _problem(20, 20, 2, 7, SMALL, True, (), seed=41)
    m = CaptionMetrics(WM, pointer_base=V)
    t, i, r = torch.from_numpy(cands).cuda(), torch.from_numpy(img).cuda(), torch.from_numpy(refs).cuda()
    with pytest.raises(IckError):
        m(t, i, torch.zeros(5, 17, 20, dtype=torch.int64).cuda())             # M = 17
    with pytest.raises(IckError):
        m(torch.zeros(7, 65, dtype=torch.int64).cuda(), i, r)                 # T = 65
    with pytest.raises(IckError):
        m(t, i, torch.zeros(5, 2, 65, dtype=torch.int64).cuda())              # Lr = 65
    with pytest.raises(IckError):
        m(t, i[:6], r)
    img2 = img.copy()
    img2[2], img2[5] = 5, -1
    got = m(t, torch.from_numpy(img2).cuda(), r)
    good = np.array([k not in (2, 5) for k in range(7)])
    assert np.isnan(got.bleu.cpu().numpy()[~good]).all() and np.isnan(got.rouge_l.cpu().numpy()[~good]).all()
    assert not got.counts.cpu().numpy()[~good].any() and not got.pointers.cpu().numpy()[~good].any()
    want = _restate(cands[good], img[good], refs)
    _check_rows([x[torch.from_numpy(good).cuda()] for x in got], want)
    res = CaptionMetrics.result(m.totals(got))                                # the totals skip the two NaN rows
    assert res["captions"] == 5
    ref = R.corpus(want)
    assert abs(res["Bleu_2"] - ref["Bleu_2"]) <= 1e-9 and res["pointer_recall"] == ref["pointer_recall"]


# ------------------------------------------------------------------------------------------------ SCST layout
def _scst_problem(B, n, M, baseline, seed, T=12):
    rng = np.random.default_rng(seed)
    refs = _rows(rng, B * M, T, SMALL, True, ()).reshape(B, M, T)
    N = B * n + (B if baseline == "greedy" else 0)
    rows = _rows(rng, N, T, SMALL, True, ())
    img = np.concatenate([np.repeat(np.arange(B), n)] + ([np.arange(B)] if baseline == "greedy" else []))
    return rows, img, refs


def _np_advantages(rewards, B, n, baseline):
    r = rewards[:B * n].reshape(B, n)
    if baseline == "greedy":
        return (r - rewards[B * n:].reshape(B, 1)).reshape(-1)
    out = np.empty_like(r)
    for b in range(B):
        s = np.float32(0)
        for k in range(n):
            s = np.float32(s + r[b, k])
        for j in range(n):
            out[b, j] = np.float32(r[b, j] - np.float32(np.float32(s - r[b, j]) / np.float32(n - 1)))
    return out.reshape(-1)


@pytest.mark.parametrize("baseline", ["greedy", "mean"])
@pytest.mark.parametrize("B,n,M", [(1, 2, 3), (3, 5, 3), (3, 2, 1), (2, 40, 1)])
def test_scst_layout_matches_general_mode(baseline, B, n, M):
    rows, img, refs = _scst_problem(B, n, M, baseline, seed=B * 100 + n)
    t, i, r = torch.from_numpy(rows).cuda(), torch.from_numpy(img).cuda(), torch.from_numpy(refs).cuda()
    m = CaptionMetrics(WM, pointer_base=V)
    weights = (0.0, 0.25, 0.0, 0.5, 1.0, 2.0)
    reward = m.reward(bleu=weights[1:5], rouge_l=weights[5])
    general = ops.caption_metrics(t, r, START, END, PAD, (), V, 1.2, image_index=i, weights=weights)
    scst = ops.caption_metrics(t, r, START, END, PAD, (), V, 1.2, num_samples=n, baseline=baseline, weights=weights)
    for a, b in zip(general[:5], scst[:5]):
        assert torch.equal(a, b)                                              # per-row outputs and rewards: same bits
    assert general[5] is None
    rew, adv = reward.scst(t, r, n, baseline)
    assert torch.equal(rew, scst[4]) and torch.equal(adv, scst[5]) and torch.equal(reward(t, i, r), rew)
    assert np.array_equal(adv.cpu().numpy(), _np_advantages(rew.cpu().numpy(), B, n, baseline))
    # the rewards against the restatement, in float64
    want = _restate(rows, img, refs)
    _check_rows(scst, want)
    w_ref = np.array([R.reward(w, weights) for w in want])
    assert np.abs(rew.cpu().numpy() - w_ref).max() <= 1e-5 * max(1.0, np.abs(w_ref).max())
    a_ref = np.array(R.advantages(list(w_ref), B, n, baseline))
    assert np.abs(adv.cpu().numpy() - a_ref).max() <= 2e-5 * max(1.0, np.abs(w_ref).max())


@pytest.mark.parametrize("baseline", ["greedy", "mean"])
def test_cider_only_reward_gives_ciders_bits(baseline):
    B, n, M = 3, 5, 2
    rows, img, refs = _scst_problem(B, n, M, baseline, seed=7)
    t, i, r = torch.from_numpy(rows).cuda(), torch.from_numpy(img).cuda(), torch.from_numpy(refs).cuda()
    cider = CiderD(r, WM)
    c_rew, c_adv = cider.scst(t, r, n, baseline)
    reward = CaptionMetrics(WM, pointer_base=V).reward(cider=cider, cider_weight=1.0)
    rew, adv = reward.scst(t, r, n, baseline)
    assert torch.equal(rew, c_rew) and torch.equal(adv, c_adv)
    assert torch.equal(reward(t, i, r), cider(t, i, r))
    assert float(c_rew.max()) > 0.0
    # a mix: w_base * cider + w_b4 * bleu4 in fp32, in that order
    mix = CaptionMetrics(WM).reward(cider=cider, cider_weight=0.5, bleu=(0, 0, 0, 2.0))
    rows4 = CaptionMetrics(WM)(t, i, r)
    want = np.float32(0.5) * c_rew.cpu().numpy() + np.float32(0.0) * rows4.bleu[:, 0].cpu().numpy()
    want = want + np.float32(0.0) * rows4.bleu[:, 1].cpu().numpy() + np.float32(0.0) * rows4.bleu[:, 2].cpu().numpy()
    want = want + np.float32(2.0) * rows4.bleu[:, 3].cpu().numpy() + np.float32(0.0) * rows4.rouge_l.cpu().numpy()
    assert np.array_equal(mix.scst(t, r, n, baseline)[0].cpu().numpy(), want.astype(np.float32))


# ------------------------------------------------------------------------------------------------ totals
def test_totals_and_corpus_result():
    cands, img, refs = _problem(20, 20, 5, 130, SMALL, True, (), seed=50)
    m = CaptionMetrics(WM, pointer_base=V)
    t, i, r = torch.from_numpy(cands).cuda(), torch.from_numpy(img).cuda(), torch.from_numpy(refs).cuda()
    rows = m(t, i, r)
    tot = m.totals(rows)
    assert tot.sums.dtype == torch.int64 and tot.sums.shape == (14,) and tot.rouge_sum.dtype == torch.float64
    sums = tot.sums.cpu().numpy()
    assert np.array_equal(sums[:10], rows.counts.cpu().numpy().astype(np.int64).sum(0))
    assert np.array_equal(sums[10:13], rows.pointers.cpu().numpy().astype(np.int64).sum(0)) and sums[13] == 130
    rs = rows.rouge_l.cpu().numpy().astype(np.float64).sum()
    assert abs(tot.rouge_sum.item() - rs) <= 1e-12 * rs
    again = m.totals(m(t, i, r))
    assert torch.equal(again.sums, tot.sums) and torch.equal(again.rouge_sum, tot.rouge_sum)        # same bits
    both = tot + again                                                        # a device add of two batches
    assert torch.equal(both.sums, 2 * tot.sums) and both.rouge_sum.item() == 2 * tot.rouge_sum.item()
    want = _restate(cands, img, refs)
    res, ref = CaptionMetrics.result(tot), R.corpus(want)
    assert set(res) == set(ref) and res["captions"] == 130 and ref["pointer_precision"] > 0 and ref["Bleu_4"] > 0.01
    for k in ("Bleu_1", "Bleu_2", "Bleu_3", "Bleu_4", "pointer_precision", "pointer_recall"):
        assert abs(res[k] - ref[k]) <= 1e-9, (k, res[k], ref[k])
    rouge32 = np.mean([np.float64(np.float32(w.rouge_l)) for w in want])      # the rows hold float32
    assert abs(res["ROUGE_L"] - rouge32) <= 1e-9 and abs(res["ROUGE_L"] - ref["ROUGE_L"]) <= 6e-8
    twice = CaptionMetrics.result(both)       # (not the same bits: the formula's 1e-15 and 1e-9 do not double)
    assert abs(twice["Bleu_4"] - res["Bleu_4"]) <= 1e-9 and twice["captions"] == 260


# ------------------------------------------------------------------------------------------------ SelfCriticalStep
WEIGHTS = (1.0, 0.1, 0.0, 0.0, 0.5, 0.3)


def _mixed(refs, wm, pointer_base):
    cider = CiderD(refs, wm)
    reward = CaptionMetrics(wm, pointer_base=pointer_base).reward(cider=cider, cider_weight=WEIGHTS[0],
                                                                  bleu=WEIGHTS[1:5], rouge_l=WEIGHTS[5])
    return cider, reward


@pytest.mark.parametrize("variant,baseline", [("geo", "greedy"), ("knowledge", "mean")])
def test_scst_with_metric_reward_matches_host_twin(variant, baseline):
    B, Vs, K = 3, 40, 5
    wm = synth.make_word_map(Vs)
    refs = _refs_for(B, Vs, K, seed=2)
    cider, reward = _mixed(refs, wm, Vs)
    keys, counts, lrl = cider.table()
    df = table_to_dict(keys, counts)
    ref_rows = [list(r) for r in refs.numpy()]

    def host_reward(toks, img):
        base = cider_rows(toks.numpy(), img.numpy(), ref_rows, df, lrl, wm["<start>"], wm["<end>"], wm["<pad>"])
        rows = R.caption_rows(toks.numpy(), img.numpy(), ref_rows, wm["<start>"], wm["<end>"], wm["<pad>"])
        return [R.reward(r, WEIGHTS, b) for r, b in zip(rows, base)]

    dev_step, dev_ts, _, ents, facts, enc = _twin(variant, reward, baseline=baseline)
    host_step, host_ts, _, _, _, _ = _twin(variant, host_reward, baseline=baseline)
    args = [enc.cuda(), ents] + ([facts.cuda()] if facts is not None else [])
    for k in range(2):
        a = dev_step(*args, refs=refs.cuda())
        h = host_step(*args)
        assert a.samples.is_cuda and a.rewards.is_cuda and a.advantages.is_cuda
        assert torch.equal(a.samples.cpu(), h.samples), k
        for got, want in ((a.rewards, h.rewards), (a.advantages, h.advantages)):
            err = (got.cpu().double() - want.double()).abs().max().item()
            assert err <= 1e-5 * max(1.0, want.abs().max().item()), (k, err)
        assert abs(a.loss.item() - h.loss.item()) < 2e-5, (a.loss.item(), h.loss.item())
        torch.cuda.synchronize()
        err = (dev_ts.flat_p - host_ts.flat_p).abs().max().item()
        assert err < 5e-5, (k, err)
    assert float(h.rewards.max()) > 0.0


def test_scst_metric_reward_step_copies_nothing_to_the_host(monkeypatch):
    Vs, K = 40, 5
    refs = _refs_for(3, Vs, K).cuda()
    _, reward = _mixed(refs, synth.make_word_map(Vs), Vs)
    step, ts, dec, ents, facts, enc = _twin("knowledge", reward)
    args = [enc.cuda(), ents.cuda(), facts.cuda()]
    with pytest.raises(IckError):
        step(*args)                                                           # a MetricReward needs refs
    step(*args, refs=refs)                                                    # warm-up: graph captures
    torch.cuda.synchronize()

    def no_host(*a, **k):
        raise AssertionError("device-to-host copy inside the SCST step")

    for name in ("cpu", "item", "tolist", "numpy"):
        monkeypatch.setattr(torch.Tensor, name, no_host)
    out = step(*args, refs=refs)
    monkeypatch.undo()
    torch.cuda.synchronize()
    assert torch.isfinite(out.loss).all() and out.rewards.shape == (9,) and out.advantages.shape == (9,)


def test_cider_reward_keeps_its_bits_beside_a_metric_reward():
    Vs, K = 40, 5
    wm = synth.make_word_map(Vs)
    refs = _refs_for(3, Vs, K, seed=2)

    def run():
        step, _, _, ents, _, enc = _twin("geo", CiderD(refs, wm))
        out = step(enc.cuda(), ents, refs=refs.cuda())
        torch.cuda.synchronize()
        return out

    before = run()
    _, reward = _mixed(refs, wm, Vs)
    assert isinstance(reward, MetricReward)
    reward.scst(torch.cat([before.samples, before.greedy]), refs.cuda(), 3, "greedy")
    after = run()
    for a, b in ((before.samples, after.samples), (before.greedy, after.greedy), (before.rewards, after.rewards),
                 (before.greedy_rewards, after.greedy_rewards), (before.advantages, after.advantages)):
        assert torch.equal(a, b)


# ------------------------------------------------------------------------------------------------ train.py, eval.py
@pytest.fixture(scope="module")
def toy(tmp_path_factory):
    """A synthetic data set and a one-epoch checkpoint on it, trained with val_caption_metrics on."""
    import ick_amd.train as tr
    root = tmp_path_factory.mktemp("metrics")
    data_dir = str(root / "data")
    wm = synth.write_dataset(data_dir, "toy", "geo", n_train=24, n_val=8, n_test=4, L=12, K=6, V=60)
    base = dict(variant="geo", data_dir=data_dir, data_name="toy", batch_size=4, workers=0, print_freq=1000, seed=3,
                out_dir=str(root))
    torch.manual_seed(0)
    tr.STATS.pop("caption_metrics", None)
    hist = tr.main(tr.Config(epochs=1, val_caption_metrics=True, **base))
    return dict(root=root, data_dir=data_dir, wm=wm, base=base, hist=hist, stats=dict(tr.STATS["caption_metrics"]))


def _val_batches(toy):
    from ick_amd.datasets import CaptionDataset
    return torch.utils.data.DataLoader(CaptionDataset(toy["data_dir"], "toy", "VAL"), batch_size=4, shuffle=False)


def test_validate_with_caption_metrics(toy, capsys):
    import ick_amd.train as tr
    import ick_amd.utils as ut
    assert len(toy["hist"]) == 1 and math.isfinite(toy["hist"][0][1]) and toy["stats"]["captions"] == 8
    ck = ut.load_checkpoint(str(toy["root"] / "checkpoint_0_toy.pth.tar"), map_location="cuda")
    dec, enc = ck["decoder"].cuda(), ck["encoder"].cuda()
    wm = toy["wm"]
    crit = tr.make_criteria(wm["<pad>"])[1].cuda()
    dev = torch.device("cuda", torch.cuda.current_device())
    plain = tr.validate(_val_batches(toy), enc, dec, crit, tr.Config(**toy["base"]), dev)
    assert isinstance(plain, float)                                           # the default returns what it did
    capsys.readouterr()
    loss, res = tr.validate(_val_batches(toy), enc, dec, crit, tr.Config(val_caption_metrics=True, **toy["base"]), dev)
    assert abs(loss - plain) < 1e-6 and "Bleu_4" in capsys.readouterr().out
    loss_t, res_t = tr.validate(_val_batches(toy), enc, dec, crit,
                                tr.Config(val_caption_metrics=True, val_token_metrics=True, **toy["base"]), dev)
    assert res_t == res and abs(loss_t - plain) < 1e-4
    # the restatement on the captions the decoder writes for the same batches
    want = []
    with torch.no_grad():
        for batch in _val_batches(toy):
            seq = dec.predict(enc(batch[0].cuda().float()), 12, batch[4]).t().cpu().numpy()
            want += R.caption_rows(seq, range(len(seq)), [[c] for c in batch[1].numpy()], wm["<start>"], wm["<end>"],
                                   wm["<pad>"], (), len(wm))
    ref = R.corpus(want)
    assert res["captions"] == 8 and set(res) == set(ref)
    for k in ref:
        tol = 6e-8 if k == "ROUGE_L" else 1e-9
        assert abs(res[k] - ref[k]) <= tol, (k, res[k], ref[k])
    assert res == toy["stats"]                                                # what main()'s own pass recorded


def test_evaluate_with_caption_metrics(toy):
    import pandas as pd
    import ick_amd.eval as ev
    import ick_amd.utils as ut
    from ick_amd.datasets import CaptionDataset
    ck = ut.load_checkpoint(str(toy["root"] / "checkpoint_0_toy.pth.tar"), map_location="cuda")
    dec, enc = ck["decoder"].cuda().eval(), ck["encoder"].cuda().eval()
    wm = toy["wm"]
    ds = CaptionDataset(toy["data_dir"], "toy", "TEST")
    loader = lambda: torch.utils.data.DataLoader(ds, batch_size=2, shuffle=False)
    out_dir = toy["root"] / "eval"
    os.makedirs(out_dir)
    csv = str(out_dir / "generated_captions.csv")
    caps0, seqs0 = ev.evaluate(enc, dec, loader(), wm, max_caption_len=10, out_csv=csv)             # the defaults
    assert not os.path.exists(out_dir / "metric_scores_for_generated_captions.csv")
    plain_csv = open(csv).read()
    m = CaptionMetrics(wm, pointer_base=len(wm))
    refs_of = lambda bi, batch: batch[1].unsqueeze(1)                         # (B, 1, L): the image's own caption
    with pytest.raises(ValueError):
        ev.evaluate(enc, dec, loader(), wm, max_caption_len=10, out_csv=csv, metrics=m)
    caps, seqs, res = ev.evaluate(enc, dec, loader(), wm, max_caption_len=10, out_csv=csv, metrics=m, refs=refs_of)
    assert caps == caps0 and seqs == seqs0 and open(csv).read() == plain_csv
    all_refs = [[c] for c in np.asarray(ds.captions)]
    want = R.caption_rows(seqs, range(4), all_refs, wm["<start>"], wm["<end>"], wm["<pad>"], (), len(wm))
    ref = R.corpus(want)
    for k in ref:
        assert abs(res[k] - ref[k]) <= (6e-8 if k == "ROUGE_L" else 1e-9), (k, res[k], ref[k])
    df = pd.read_csv(out_dir / "metric_scores_for_generated_captions.csv")
    assert list(df.columns) == ["generated_caption", "Bleu_1", "Bleu_2", "Bleu_3", "Bleu_4", "ROUGE_L", "pointer_hits",
                                "pointer_generated", "pointer_reference"] and len(df) == 4
    _close(df["Bleu_1"].to_numpy(), [w.bleu[0] for w in want])
    assert df["pointer_reference"].tolist() == [w.pointers[2] for w in want]
    # sampled rows are scored against their image's references through image_index
    caps_s, seqs_s, res_s = ev.evaluate(enc, dec, loader(), wm, max_caption_len=10, out_csv=csv, metrics=m, refs=refs_of,
                                        sample=dict(num_samples=3, seed=5))
    want_s = R.caption_rows(seqs_s, np.repeat(np.arange(4), 3), all_refs, wm["<start>"], wm["<end>"], wm["<pad>"], (),
                            len(wm))
    ref_s = R.corpus(want_s)
    assert res_s["captions"] == 12 and abs(res_s["Bleu_1"] - ref_s["Bleu_1"]) <= 1e-9
    df = pd.read_csv(out_dir / "metric_scores_for_generated_captions.csv")
    assert list(df.columns)[:3] == ["image", "sample", "generated_caption"] and len(df) == 12
    assert df["pointer_generated"].tolist() == [w.pointers[1] for w in want_s]


def test_train_main_scst_with_a_mixed_reward(toy, capsys):
    import ick_amd.train as tr
    xe = str(toy["root"] / "checkpoint_0_toy.pth.tar")
    base = dict(toy["base"], print_freq=1, out_dir=str(toy["root"] / "scst"))
    os.makedirs(base["out_dir"])
    with pytest.raises(ValueError):
        tr.main(tr.Config(epochs=2, scst_reward=dict(bleu=(0, 0, 0, 0.5)), checkpoint=xe, **base))   # needs scst=True
    tr.STATS.pop("scst_rewards", None)
    capsys.readouterr()
    hist = tr.main(tr.Config(epochs=2, scst=True, scst_samples=3, scst_reward=dict(bleu=(0, 0, 0, 0.5)),
                             val_caption_metrics=True, checkpoint=xe, **base))
    printed = capsys.readouterr().out
    assert len(hist) == 1 and math.isfinite(hist[0][0]) and math.isfinite(hist[0][1])
    assert "reward sample" in printed and "CIDEr-D sample" not in printed
    res = tr.STATS["caption_metrics"]
    assert res["captions"] == 8 and 0.0 <= res["CIDEr-D"] <= 10.0 and 0.0 <= res["Bleu_1"] <= 1.0
    for _, _, r_s, r_g in tr.STATS["scst_rewards"]:
        assert 0.0 <= r_s <= 10.5 and 0.0 <= r_g <= 10.5
