"""Caption scoring without a GPU: the numpy restatement (tests/score_ref.py) against torch's stable sort, the rank interval
against the float32 oracle, score_captions' argument checker, and the two new C-ABI names."""
import os
import re

import numpy as np
import pytest
import torch

import ick_amd.synth as synth
from decode_ref import float64_default, params64
from ick_amd.decoder import check_score_args
from ick_amd.lib import IckError
from oracle import restatement as R
from score_ref import rank_interval, row_stats, score_batch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 2e-4
EPS = 2 * TOL


def test_rank_is_the_place_in_a_stable_descending_sort():
    rng = np.random.default_rng(0)
    for Vx in (1, 2, 7, 64, 300):
        for _ in range(8):
            s = rng.integers(-4, 5, Vx).astype(np.float32) / 4          # few distinct values: exact ties everywhere
            order = torch.argsort(-torch.from_numpy(s), stable=True).tolist()
            for target in {0, Vx - 1, int(rng.integers(0, Vx)), int(np.argmax(s))}:
                lp, rank, best = row_stats(s, target)
                assert rank == order.index(target), (Vx, target)
                assert best == order[0]
                want = torch.log_softmax(torch.from_numpy(s).double(), 0)[target].item()
                assert abs(lp - want) < 1e-12
    s = np.array([1.0, 3.0, 3.0, 2.0, 3.0], np.float32)                  # three tied maxima: ranks 0, 1, 2 by column
    assert [row_stats(s, c)[1] for c in (1, 2, 4)] == [0, 1, 2] and row_stats(s, 3)[1] == 3 and row_stats(s, 0)[1] == 4


def test_interval_holds_the_float32_oracles_rank():
    """The oracle in float32 against itself in float64: every scored row's float32 rank lies in the fp64 interval."""
    variant, B, L, K, V, seed = "geo", 3, 7, 4, 120, 2
    P = synth.make_params(variant, V, seed)
    cfg = R.config_from_word_map(variant, synth.make_word_map(V))
    batch = synth.make_batch(variant, B, L, K, V, 0, seed)
    enc = synth.make_enc_out(B, seed)
    args = (batch["captions"], enc, batch["caption_masks"], batch["caption_lengths"], batch["entities"])
    with torch.no_grad():
        s32, caps, dl = R.forward(cfg, P, *args)
        with float64_default():
            s64, caps64, _ = R.forward(cfg, params64(P), args[0], enc.double(), args[2], args[3], args[4].double())
    assert torch.equal(caps, caps64) and (s32.double() - s64).abs().max().item() < TOL
    lengths = [d + 1 for d in dl]
    got = score_batch(s32.numpy(), caps.numpy(), lengths, cfg.pad)
    ref = score_batch(s64.numpy(), caps.numpy(), lengths, cfg.pad, eps=EPS)
    ok = ref["rank"] >= 0
    assert ok.sum() == sum(dl) and np.array_equal(ok, got["rank"] >= 0)
    assert np.all(ref["lo"][ok] <= got["rank"][ok]) and np.all(got["rank"][ok] <= ref["hi"][ok])
    assert np.all(ref["lo"][ok] <= ref["rank"][ok]) and np.all(ref["rank"][ok] <= ref["hi"][ok])
    # a planted near-tie: two columns 1e-5 apart may swap under an error of TOL each, and the interval allows exactly that
    s = np.array([0.0, 1.0, 1.0 + 1e-5, -3.0])
    assert rank_interval(s, 1, EPS) == (0, 1) and rank_interval(s, 3, EPS) == (3, 3)


def _args(R_=4, L=6, B=None, K=3, F=None, dim4=False):
    B = R_ if B is None else B
    caps = torch.zeros(R_, L, dtype=torch.int64)
    enc = torch.zeros(B, 8, 14, 14) if dim4 else torch.zeros(B, 8, 5)
    d = dict(captions=caps, encoder_out=enc, caption_masks=torch.zeros_like(caps),
             caption_lengths=torch.full((R_, 1), L), entities=torch.zeros(B, K, 5), facts=None, image_index=None, top_k=5)
    if F is not None:
        d["facts"] = torch.zeros(B, F, 3, dtype=torch.int64)
    return d


def _check(has_facts, d):
    return check_score_args("score_captions", has_facts, d["captions"], d["encoder_out"], d["caption_masks"],
                            d["caption_lengths"], d["entities"], d["facts"], d["image_index"], d["top_k"])


def test_argument_checker():
    assert _check(False, _args()) == (4, 6, 4)
    assert _check(True, _args(F=2)) == (4, 6, 4)
    assert _check(False, _args(dim4=True)) == (4, 6, 4)
    ok = _args(R_=7, B=3)
    ok["image_index"] = torch.tensor([0, 0, 1, 1, 1, 2, 2])
    assert _check(False, ok) == (7, 6, 3)
    bad = []
    for k in (0, -1, True, 2.0, None):
        bad.append(dict(_args(), top_k=k))
    bad.append(dict(_args(), captions=torch.zeros(4, dtype=torch.int64)))                 # not 2-D
    bad.append(dict(_args(L=1)))                                                        # nothing to score
    bad.append(dict(_args(), caption_masks=torch.zeros(4, 5, dtype=torch.int64)))
    bad.append(dict(_args(), caption_lengths=torch.zeros(3, 1, dtype=torch.int64)))
    bad.append(dict(_args(), encoder_out=torch.zeros(4, 8)))
    bad.append(dict(_args(), entities=torch.zeros(3, 3, 5)))
    bad.append(dict(_args(), entities=torch.zeros(4, 5)))
    bad.append(dict(_args(R_=7, B=3)))                                                  # 7 captions, 3 images, no index
    bad.append(dict(ok, image_index=torch.tensor([0, 1, 2])))                           # wrong shape
    bad.append(dict(ok, image_index=torch.zeros(7)))                                    # not an integer tensor
    bad.append(dict(ok, image_index=[0, 0, 1, 1, 1, 2, 2]))                             # not a tensor
    bad.append(dict(ok, encoder_out=torch.zeros(3, 8, 14, 14)))                         # feature map + image_index
    for d in bad:
        with pytest.raises(IckError):
            _check(False, d)
    for d in (_args(), dict(_args(F=2), facts=torch.zeros(4, 2, 2, dtype=torch.int64)),
              dict(_args(F=2), facts=torch.zeros(3, 2, 3, dtype=torch.int64))):
        with pytest.raises(IckError):
            _check(True, d)


def test_abi_names_are_declared_and_bound():
    import ick_amd.lib as L
    src = open(os.path.join(ROOT, "include", "ick_amd.h")).read()
    declared = set(re.findall(r"^int\s+(ick_[a-z0-9_]+)\s*\(", src, flags=re.M))
    for name in ("ick_row_logprob_rank", "ick_caption_score_sums"):
        assert name in declared and name in L.SIGNATURES
        assert L.SIGNATURES[name][-1] is L.vp            # every launch takes the stream last
    assert sorted(L.SIGNATURES) == sorted(declared)
