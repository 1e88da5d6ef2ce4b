"""The device CIDEr-D (ick_cider_d, ick_amd.CiderD) on the GPU: the kernel against the plain-Python restatement in
general and SCST-layout mode, the corpus score of from_refs, SelfCriticalStep with a CiderD reward against a twin step
whose host reward_fn wraps the restatement, a step without any device-to-host copy, an SCST run that raises the greedy
captions' CIDEr-D, and the training script's SCST mode."""
import math
import os

import numpy as np
import pytest
import torch

import ick_amd.synth as synth
from ick_amd.cider import CiderD
from ick_amd.lib import IckError
from ick_amd.scst import SelfCriticalStep
from ick_amd.training import TrainStep
from cider_ref import cider_rows, doc_freq, table_to_dict
from test_sample_gpu import make_case
from test_training_gpu import zero_dropout

pytestmark = pytest.mark.gpu


def _tol(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    err = np.abs(got - want)
    assert (err <= 2e-5 * np.maximum(1.0, np.abs(want))).all(), (err.max(), got, want)


def _caption(rng, n_words, vocab, V, K, L, end, pad, start=None, ptr=0.1):
    ws = rng.choice(vocab, size=n_words)
    ws = np.where(rng.random(n_words) < ptr, V + rng.integers(0, K, size=n_words), ws)
    row = ([start] if start is not None else []) + list(ws) + [end]
    row = row[:L]
    return row + [pad] * (L - len(row))


def _case(V, M, T, seed, N_img=24, extra_corpus=150, K=20):
    """A reference block (N_img, M, Lr) drawn from a small Zipf-like word set (many shared n-grams), a corpus that holds
    it plus unrelated captions, and candidate rows covering the edge cases."""
    wm = synth.make_word_map(V)
    start, end, pad = wm["<start>"], wm["<end>"], wm["<pad>"]
    rng = np.random.default_rng(seed)
    vocab = np.concatenate([np.arange(1, 25), rng.integers(25, V - 3, size=40)])
    Lr = min(T, 24) + 2
    refs = np.array([[_caption(rng, int(rng.integers(1, Lr - 2)), vocab, V, K, Lr, end, pad, start)
                      for _ in range(M)] for _ in range(N_img)], dtype=np.int64)
    others = np.array([[_caption(rng, int(rng.integers(3, Lr - 2)), vocab, V, K, Lr, end, pad, start)
                        for _ in range(M)] for _ in range(extra_corpus)], dtype=np.int64).reshape(-1, M, Lr)
    corpus = np.concatenate([refs, others])
    cands, img = [], []
    for b in range(N_img):
        for kind in range(6):
            if kind == 0:                                   # one of its references, re-padded to T
                w = [t for t in refs[b, 0] if t not in (start, pad)]
                row = (w + [pad] * T)[:T]
            elif kind == 1:                                 # no <end>: all T tokens count
                row = list(rng.choice(vocab, size=T))
            elif kind == 2:                                 # empty
                row = [end] + [pad] * (T - 1)
            elif kind == 3:                                 # n-grams unseen in the corpus
                row = _caption(rng, min(T - 1, 8), np.arange(V - 200, V - 3), V, K, T, end, pad, ptr=0.0)
            elif kind == 4:                                 # heavy repetition
                row = [int(vocab[0])] * (T - 3) + [int(vocab[1]), int(vocab[0]), end][:3]
            else:                                           # a random caption with <pad> gaps and pointer ids
                row = _caption(rng, int(rng.integers(1, T)), vocab, V, K, T, end, pad)
                row[0:1] = [pad] if T > 4 else row[0:1]
            cands.append(row[:T])
            img.append(b)
    return wm, corpus, refs, np.array(cands, dtype=np.int64), np.array(img, dtype=np.int64)


def _restated(cider, wm, tokens, img, refs, ignore=()):
    keys, counts, lrl = cider.table()
    df = table_to_dict(keys, counts)
    return cider_rows(tokens, img, [list(r) for r in refs], df, lrl, wm["<start>"], wm["<end>"], wm["<pad>"], ignore)


# ------------------------------------------------------------------------------------------------ kernel vs restatement
@pytest.mark.parametrize("V,M,T", [(10000, 1, 20), (10000, 5, 64), (50000, 5, 20), (50000, 1, 64)])
def test_general_mode_matches_restatement(V, M, T):
    wm, corpus, refs, cands, img = _case(V, M, T, seed=V + M + T)
    ignore = (7,) if M == 5 else ()
    cider = CiderD(torch.from_numpy(corpus), wm, ignore=ignore)
    keys, counts, lrl = cider.table()
    df_ref, lrl_ref = doc_freq([list(c) for c in corpus], wm["<start>"], wm["<end>"], wm["<pad>"], ignore)
    assert table_to_dict(keys, counts) == df_ref and lrl == lrl_ref
    t, i, r = torch.from_numpy(cands).cuda(), torch.from_numpy(img).cuda(), torch.from_numpy(refs).cuda()
    got = cider(t, i, r)
    want = _restated(cider, wm, cands, img, refs, ignore)
    _tol(got.cpu().numpy(), want)
    assert max(want) > 1.0 and min(want) == 0.0                       # both ends of the range were exercised
    again = cider(t, i, r)
    assert torch.equal(got, again)                                      # bit-identical


def test_out_of_range_image_index_gives_nan():
    wm, corpus, refs, cands, img = _case(10000, 1, 20, seed=5, N_img=4, extra_corpus=10)
    cider = CiderD(torch.from_numpy(corpus), wm)
    img[3] = 4
    got = cider(torch.from_numpy(cands).cuda(), torch.from_numpy(img).cuda(), torch.from_numpy(refs).cuda()).cpu()
    assert math.isnan(got[3]) and not torch.isnan(got[:3]).any() and not torch.isnan(got[4:]).any()


def test_from_refs_corpus_score():
    wm, _, refs, cands, img = _case(10000, 5, 20, seed=9, N_img=20, extra_corpus=0)
    cands = cands[::6]                                                  # one candidate per image
    cider = CiderD.from_refs(torch.from_numpy(refs).cuda(), wm)
    score = cider(torch.from_numpy(cands).cuda(), torch.arange(20).cuda(), torch.from_numpy(refs).cuda()).mean()
    df, lrl = doc_freq([list(r) for r in refs], wm["<start>"], wm["<end>"], wm["<pad>"])
    want = np.mean(cider_rows(cands, range(20), [list(r) for r in refs], df, lrl, wm["<start>"], wm["<end>"],
                              wm["<pad>"]))
    assert want > 0.5 and abs(score.item() - want) < 2e-5 * max(1.0, want)


@pytest.mark.parametrize("baseline", ["greedy", "mean"])
def test_scst_layout_rewards_and_advantages(baseline):
    V, M, T, n = 10000, 3, 20, 5
    wm, corpus, refs, cands, _ = _case(V, M, T, seed=17, N_img=8)
    B = refs.shape[0]
    rng = np.random.default_rng(1)
    rows = cands[rng.integers(0, cands.shape[0], size=B * n + (B if baseline == "greedy" else 0))]
    img = np.concatenate([np.repeat(np.arange(B), n)] + ([np.arange(B)] if baseline == "greedy" else []))
    cider = CiderD(torch.from_numpy(corpus), wm)
    r, adv = cider.scst(torch.from_numpy(rows).cuda(), torch.from_numpy(refs).cuda(), n, baseline)
    want = np.array(_restated(cider, wm, rows, img, refs))
    _tol(r.cpu().numpy(), want)
    rs = want[:B * n].reshape(B, n)
    if baseline == "greedy":
        a_ref = rs - want[B * n:].reshape(B, 1)
    else:
        a_ref = rs - (rs.sum(1, keepdims=True) - rs) / (n - 1)
    _tol(adv.cpu().numpy(), a_ref.reshape(-1))
    r2, adv2 = cider.scst(torch.from_numpy(rows).cuda(), torch.from_numpy(refs).cuda(), n, baseline)
    assert torch.equal(r, r2) and torch.equal(adv, adv2)


# ------------------------------------------------------------------------------------------------ SelfCriticalStep
def _refs_for(B, V, K, M=2, L=10, seed=0):
    rng = np.random.default_rng(seed)
    wm = synth.make_word_map(V)
    return torch.from_numpy(np.array([[_caption(rng, int(rng.integers(3, L - 2)), np.arange(1, V - 3), V, K, L,
                                                wm["<end>"], wm["<pad>"], wm["<start>"], ptr=0.2)
                                       for _ in range(M)] for _ in range(B)], dtype=np.int64))


def _twin(variant, reward, baseline="greedy", B=3, n=3, V=40, K=5, T=8, lr=4e-4):
    dec, cfg, P, ents, facts, enc = make_case(variant, B, K, V, 4, 21, end_bias=1.5)
    dec = zero_dropout(dec.train())
    ts = TrainStep(dec, lr=lr, grad_clip=5.0)
    return SelfCriticalStep(ts, reward, num_samples=n, baseline=baseline, max_len=T, seed=3), ts, dec, ents, facts, enc


@pytest.mark.parametrize("variant", ["geo", "knowledge"])
def test_scst_with_cider_matches_host_twin(variant):
    B, V, K = 3, 40, 5
    wm = synth.make_word_map(V)
    refs = _refs_for(B, V, K, seed=2)
    cider = CiderD(refs, wm)
    keys, counts, lrl = cider.table()
    df = table_to_dict(keys, counts)
    ref_rows = [list(r) for r in refs.numpy()]

    def host_reward(toks, img):
        return cider_rows(toks.numpy(), img.numpy(), ref_rows, df, lrl, wm["<start>"], wm["<end>"], wm["<pad>"])

    dev_step, dev_ts, dev_dec, ents, facts, enc = _twin(variant, cider)
    host_step, host_ts, host_dec, _, _, _ = _twin(variant, host_reward)
    args = [enc.cuda(), ents] + ([facts.cuda()] if facts is not None else [])
    for k in range(2):
        a = dev_step(*args, refs=refs.cuda())
        h = host_step(*args)
        assert a.samples.is_cuda and a.rewards.is_cuda and a.advantages.is_cuda and a.greedy.is_cuda
        assert torch.equal(a.samples.cpu(), h.samples) and torch.equal(a.greedy.cpu(), h.greedy), k
        _tol(a.rewards.cpu().numpy(), h.rewards.numpy())
        _tol(a.greedy_rewards.cpu().numpy(), h.greedy_rewards.numpy())
        _tol(a.advantages.cpu().numpy(), h.advantages.numpy())
        assert abs(a.loss.item() - h.loss.item()) < 2e-5, (a.loss.item(), h.loss.item())
        torch.cuda.synchronize()
        err = (dev_ts.flat_p - host_ts.flat_p).abs().max().item()
        assert err < 5e-5, (k, err)
    assert float(h.rewards.max()) > 0.0                                 # a reward that is not all zero
    assert dev_step.captures == 2 and host_step.captures == 2


def test_scst_reward_argument_errors():
    V, K = 40, 5
    refs = _refs_for(3, V, K)
    cider = CiderD(refs, synth.make_word_map(V))
    step, ts, dec, ents, facts, enc = _twin("geo", cider)
    with pytest.raises(IckError):
        step(enc.cuda(), ents)                                          # a CiderD needs refs
    host, *_ = _twin("geo", lambda t, i: t.sum(1))
    with pytest.raises(IckError):
        host(enc.cuda(), ents, refs=refs.cuda())                        # refs with a host reward_fn
    with pytest.raises(IckError):
        step(enc.cuda(), ents, refs=_refs_for(4, V, K).cuda())          # refs for another batch size


def test_scst_cider_step_copies_nothing_to_the_host(monkeypatch):
    V, K = 40, 5
    refs = _refs_for(3, V, K).cuda()
    cider = CiderD(refs, synth.make_word_map(V))
    step, ts, dec, ents, facts, enc = _twin("knowledge", cider)
    args = [enc.cuda(), ents.cuda(), facts.cuda()]
    step(*args, refs=refs)                                              # warm-up: graph captures
    torch.cuda.synchronize()

    def no_host(*a, **k):
        raise AssertionError("device-to-host copy inside the SCST step")

    for name in ("cpu", "item", "tolist", "numpy"):
        monkeypatch.setattr(torch.Tensor, name, no_host)
    out = step(*args, refs=refs)
    monkeypatch.undo()
    torch.cuda.synchronize()
    assert torch.isfinite(out.loss).all() and out.rewards.shape == (9,) and out.advantages.shape == (9,)


def test_scst_with_cider_raises_greedy_cider():
    """A tiny fixed-seed problem: every image has the same two target captions (df from a corpus of unrelated captions
    too, so their n-grams keep their idf).  SCST with the device CIDEr-D raises the greedy captions' score (the
    greedy baseline's rewards: each step scores the greedy captions of the parameters it starts from)."""
    B, V, K, T, n = 4, 40, 5, 8, 8
    wm = synth.make_word_map(V)
    start, end, pad = wm["<start>"], wm["<end>"], wm["<pad>"]
    targets = [[start, 3, 4, 5, 6, end, pad, pad, pad], [start, 3, 4, 7, 8, end, pad, pad, pad]]
    refs = torch.tensor([targets] * B, dtype=torch.int64)
    rng = np.random.default_rng(4)
    others = [[start] + list(rng.integers(1, V - 3, size=6)) + [end, pad] for _ in range(60)]
    corpus = torch.tensor([targets[0]] * B + others, dtype=torch.int64)
    cider = CiderD(corpus, wm)
    step, ts, dec, ents, facts, enc = _twin("geo", cider, B=B, n=n, T=T, lr=1e-3)
    e, r = enc.cuda(), refs.cuda()
    greedy, sampled = [], []
    for _ in range(40):
        out = step(e, ents, refs=r)
        greedy.append(out.greedy_rewards.mean().item())
        sampled.append(out.rewards.mean().item())
    before, after = np.mean(greedy[:3]), np.mean(greedy[-3:])
    print("greedy CIDEr-D first 3 steps %.3f, last 3 %.3f; sampled %.3f -> %.3f" %
          (before, after, np.mean(sampled[:3]), np.mean(sampled[-3:])))
    assert after > before + 0.5, greedy


# ------------------------------------------------------------------------------------------------ training script
def test_train_main_scst_mode(tmp_path, capsys):
    import ick_amd.train as tr
    import ick_amd.utils as ut
    data_dir = str(tmp_path / "data")
    synth.write_dataset(data_dir, "toy", "geo", n_train=24, n_val=8, n_test=4, L=12, K=6, V=60)
    base = dict(variant="geo", data_dir=data_dir, data_name="toy", batch_size=8, workers=0, print_freq=1, seed=3)
    torch.manual_seed(0)
    tr.main(tr.Config(epochs=1, out_dir=str(tmp_path), **base))
    xe = str(tmp_path / "checkpoint_0_toy.pth.tar")
    with pytest.raises(ValueError):
        tr.main(tr.Config(epochs=2, scst=True, fused=False, checkpoint=xe, out_dir=str(tmp_path), **base))
    tr.STATS.pop("scst_rewards", None)
    capsys.readouterr()
    hist = tr.main(tr.Config(epochs=3, scst=True, scst_samples=3, checkpoint=xe, out_dir=str(tmp_path), **base))
    printed = capsys.readouterr().out
    assert len(hist) == 2 and all(math.isfinite(h[0]) and math.isfinite(h[1]) for h in hist)   # epochs 1 and 2
    for name in ("checkpoint_toy.pth.tar", "checkpoint_2_toy.pth.tar"):
        assert os.path.exists(tmp_path / name), name
    ck = ut.load_checkpoint(str(tmp_path / "checkpoint_2_toy.pth.tar"), map_location="cuda")
    assert ck["epoch"] == 2
    logged = tr.STATS["scst_rewards"]
    assert len(logged) == 6 and "CIDEr-D sample" in printed                # 3 batches x 2 epochs, print_freq 1
    for _, _, r_s, r_g in logged:
        assert 0.0 <= r_s <= 10.0 and 0.0 <= r_g <= 10.0
