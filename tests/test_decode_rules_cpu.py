"""CPU checks of the decoding rules (length penalty, no-repeat n-gram, min length): the CPU
restatement's banned set against brute-force n-gram enumeration, the length-penalty table, the rules beam search with
every rule off against the oracle's beam search, argument errors and the ABI struct layout."""
import ctypes
import os
import random
import subprocess
import tempfile

import pytest
import torch

import ick_amd
import ick_amd.synth as synth
from ick_amd.lib import IckError
from oracle import restatement as R
from beam_rules_ref import banned_brute, banned_set, has_banned_ngram, lp_table, predict_beam_rules

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def built_lib():
    import ick_amd.build as build
    return build.build()


def test_banned_set_matches_brute_force():
    rng = random.Random(5)
    end = 9
    for _ in range(400):
        t = rng.randrange(0, 30)
        seq = [rng.randrange(0, 6) for _ in range(t)]        # a small alphabet: many repeats
        n, m = rng.randrange(0, 9), rng.randrange(0, 12)
        assert banned_set(seq, t, n, m, end) == banned_brute(seq, t, n, m, end), (seq, t, n, m)


def test_banned_set_examples():
    end = 99
    assert banned_set([], 0, 3, 0, end) == set()
    assert banned_set([1, 2, 3], 3, 1, 0, end) == {1, 2, 3}
    assert banned_set([1, 2, 3, 1], 4, 2, 0, end) == {2}                 # "1 2" seen: 2 may not follow 1 again
    assert banned_set([1, 2, 3, 1, 2], 5, 3, 0, end) == {3}              # "1 2 3" seen
    assert banned_set([1, 2, 3, 1, 2], 5, 3, 6, end) == {3, end}
    assert banned_set([1, 2], 2, 0, 2, end) == set()                     # t == m: <end> allowed
    assert has_banned_ngram([1, 2, 1, 2], 2, 0, end) == 3
    assert has_banned_ngram([end], 0, 1, end) == 0
    assert has_banned_ngram([4, end], 2, 1, end) is None


def test_length_penalty_table():
    lp = lp_table(0.6, 20)
    assert lp.dtype == torch.float32 and lp.shape == (21,)
    for L in range(1, 21):
        assert lp[L].item() == float(torch.tensor(((5.0 + L) / 6.0) ** 0.6, dtype=torch.float64).float())
    assert lp[0].item() == 1.0 and lp[1].item() == 1.0
    assert torch.equal(lp_table(0.0, 7), torch.ones(8))
    assert (lp_table(1.0, 30)[1:].diff() > 0).all()


def test_rules_tensor_layout():
    import ick_amd.decoder as D
    t = D.rules_tensor(12, 0.6, 3, 5, device="cpu")
    assert t.dtype == torch.int32 and t.shape == (4 + 13,)
    assert t[:4].tolist() == [3, 5, 1, 0]
    assert torch.equal(t[4:].view(torch.float32), lp_table(0.6, 12))
    assert D.rules_tensor(12, device="cpu")[:4].tolist() == [0, 0, 0, 0]


@pytest.mark.parametrize("variant,beam", [("geo", 3), ("knowledge", 2)])
def test_rules_reference_all_off_is_oracle_beam(variant, beam):
    V, K, Fn, max_len, seed = 50, 5, 4, 6, 3
    cfg = R.config_from_word_map(variant, synth.make_word_map(V))
    P = synth.make_params(variant, V, seed)
    ents = synth.make_entities(variant, 1, K, V, seed)
    facts = synth.make_facts(variant, 1, Fn, K, seed) if variant != "geo" else None
    enc = synth.make_enc_out(1, seed)
    with torch.no_grad():
        seq, score, _ = R.predict_beam(cfg, P, enc, max_len, ents, facts, beam)
    mine, my_score, my_key, allh = predict_beam_rules(cfg, P, enc, max_len, ents, facts, beam)
    assert torch.equal(mine, seq) and my_score == score
    assert abs(my_key - score) < 1e-5 and len(allh) == beam


def test_rules_reference_applies_rules():
    variant, V, K, max_len, seed = "geo", 50, 5, 8, 3
    cfg = R.config_from_word_map(variant, synth.make_word_map(V))
    P = synth.make_params(variant, V, seed)
    ents = synth.make_entities(variant, 1, K, V, seed)
    enc = synth.make_enc_out(1, seed)
    _, _, _, allh = predict_beam_rules(cfg, P, enc, max_len, ents, None, 3, length_penalty=1.0,
                                       no_repeat_ngram_size=1, min_len=4)
    for seq, _, L in allh:
        assert len(set(seq)) == len(seq) and cfg.end not in seq[:4] and L == len(seq)


def cpu_decoder(variant="geo", V=50):
    m = ick_amd.load_models(variant)
    return m.DecoderTransformer(word_map=synth.make_word_map(V), emb_dim=300, decoder_dim=512, encoder_dim=512,
                                num_heads=10, num_layers=3)


BAD = [dict(length_penalty=-0.1), dict(length_penalty=float("nan")), dict(length_penalty=float("inf")),
       dict(length_penalty="0.6"), dict(no_repeat_ngram_size=-1), dict(no_repeat_ngram_size=9),
       dict(no_repeat_ngram_size=2.0), dict(min_len=-1), dict(min_len=13), dict(min_len=True)]


@pytest.mark.parametrize("kw", BAD, ids=lambda k: "%s=%r" % next(iter(k.items())))
def test_beam_argument_errors(kw):
    dec = cpu_decoder()
    enc = torch.zeros(1, 512, 14, 14)
    ents = synth.make_entities("geo", 1, 5, 50, 1)
    with pytest.raises(IckError):
        dec.predict_beam(enc, 12, ents, beam_size=3, **kw)


@pytest.mark.parametrize("kw", [k for k in BAD if "length_penalty" not in k],
                         ids=lambda k: "%s=%r" % next(iter(k.items())))
def test_sample_argument_errors(kw):
    dec = cpu_decoder()
    enc = torch.zeros(1, 512, 14, 14)
    ents = synth.make_entities("geo", 1, 5, 50, 1)
    with pytest.raises(IckError):
        dec.predict_sample(enc, 12, ents, num_samples=2, **kw)


def test_rules_need_more_columns_than_steps():
    dec = cpu_decoder(V=10)
    enc = torch.zeros(1, 512, 14, 14)
    ents = synth.make_entities("geo", 1, 5, 10, 1)                 # V + K = 15
    for kw in (dict(no_repeat_ngram_size=2), dict(min_len=1), dict(length_penalty=0.5)):
        with pytest.raises(IckError):
            dec.predict_beam(enc, 15, ents, beam_size=2, **kw)
    with pytest.raises(IckError):
        dec.predict_sample(enc, 16, ents, no_repeat_ngram_size=1)


def test_decode_rules_layout_matches_header(built_lib):
    import ick_amd.lib as L
    src = '#include <stdio.h>\n#include "ick_amd.h"\nint main(){printf("%zu", sizeof(ick_decode_rules));}\n'
    with tempfile.TemporaryDirectory() as td:
        c = os.path.join(td, "sz.c")
        open(c, "w").write(src)
        exe = os.path.join(td, "sz")
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
        size = int(subprocess.check_output([exe]))
    assert ctypes.sizeof(L.DecodeRules) == size == 24


def test_library_exports_rules_symbols(built_lib):
    import ick_amd.lib as L
    lib = ctypes.CDLL(built_lib)
    for s in ("ick_decode_select_beam_rules", "ick_decode_select_sample_rules"):
        assert hasattr(lib, s) and s in L.SIGNATURES
