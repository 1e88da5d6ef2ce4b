"""CPU checks of diverse beam search (predict_beam(num_beam_groups, diversity_penalty)): argument
errors, the CPU reference against the oracle's beam search (one group) and the width-k_g search (lambda = 0), a step
worked by hand, and the ABI of the new entry point."""
import ctypes
import os
import subprocess
import tempfile

import pytest
import torch

import ick_amd
import ick_amd.synth as synth
from ick_amd.lib import IckError
from oracle import restatement as R
from beam_rules_ref import lp_table, predict_beam_rules, step_logp
from diverse_beam_ref import diverse_step, group_best, predict_diverse_beam

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def built_lib():
    import ick_amd.build as build
    return build.build()


def cpu_decoder(variant="geo", V=50):
    m = ick_amd.load_models(variant)
    return m.DecoderTransformer(word_map=synth.make_word_map(V), emb_dim=300, decoder_dim=512, encoder_dim=512,
                                num_heads=10, num_layers=3)


# (beam_size, keyword arguments)
BAD = [(6, dict(num_beam_groups=0)), (4, dict(num_beam_groups=5)), (6, dict(num_beam_groups=4)),
       (6, dict(num_beam_groups=2.0)), (6, dict(num_beam_groups=True)), (6, dict(num_beam_groups="3")),
       (6, dict(num_beam_groups=3, diversity_penalty=-0.5)),
       (6, dict(num_beam_groups=3, diversity_penalty=float("nan"))),
       (6, dict(num_beam_groups=3, diversity_penalty=float("inf"))),
       (6, dict(num_beam_groups=3, diversity_penalty="1")),
       (6, dict(diversity_penalty=-1.0)), (6, dict(diversity_penalty=True)), (1, dict(num_beam_groups=2))]


@pytest.mark.parametrize("beam,kw", BAD, ids=lambda x: repr(x) if isinstance(x, dict) else "beam%d" % x)
def test_argument_errors(beam, kw):
    """Every one raises IckError before any device work (this decoder has no GPU copy of anything)."""
    dec = cpu_decoder()
    enc = torch.zeros(1, 512, 14, 14)
    ents = synth.make_entities("geo", 1, 5, 50, 1)
    with pytest.raises(IckError):
        dec.predict_beam(enc, 12, ents, beam_size=beam, **kw)


def case(variant, V=50, K=5, Fn=4, seed=3):
    cfg = R.config_from_word_map(variant, synth.make_word_map(V))
    P = synth.make_params(variant, V, seed)
    ents = synth.make_entities(variant, 1, K, V, seed)
    facts = synth.make_facts(variant, 1, Fn, K, seed) if variant != "geo" else None
    return cfg, P, ents, facts, synth.make_enc_out(1, seed)


@pytest.mark.parametrize("variant,beam", [("geo", 3), ("knowledge", 2)])
def test_one_group_is_the_oracle_beam(variant, beam):
    cfg, P, ents, facts, enc = case(variant)
    with torch.no_grad():
        seq, score, _ = R.predict_beam(cfg, P, enc, 6, ents, facts, beam)
    mine, my_score, _, groups = predict_diverse_beam(cfg, P, enc, 6, ents, facts, beam, 1, 3.0)
    assert torch.equal(mine, seq) and my_score == score and len(groups) == 1 and len(groups[0]) == beam


def test_one_group_is_the_rules_beam():
    cfg, P, ents, facts, enc = case("geo")
    kw = dict(length_penalty=0.6, no_repeat_ngram_size=2, min_len=3)
    ref = predict_beam_rules(cfg, P, enc, 8, ents, facts, 3, **kw)
    mine = predict_diverse_beam(cfg, P, enc, 8, ents, facts, 3, 1, 2.0, **kw)
    assert torch.equal(mine[0], ref[0]) and mine[1] == ref[1] and mine[2] == ref[2]
    assert [h[:3] for h in mine[3][0]] == [tuple(h) for h in ref[3]]


@pytest.mark.parametrize("variant,beam,G,rules", [("geo", 4, 2, False), ("knowledge", 6, 3, True),
                                                  ("geo", 6, 2, True)])
def test_zero_penalty_gives_copies_of_the_narrow_search(variant, beam, G, rules):
    cfg, P, ents, facts, enc = case(variant)
    kw = dict(length_penalty=0.6, no_repeat_ngram_size=2, min_len=3) if rules else {}
    kg = beam // G
    _, _, _, narrow = predict_beam_rules(cfg, P, enc, 7, ents, facts, kg, **kw)
    _, _, _, groups = predict_diverse_beam(cfg, P, enc, 7, ents, facts, beam, G, 0.0, **kw)
    for g in range(G):
        assert [h[:3] for h in groups[g]] == [tuple(h) for h in narrow], g


def test_penalty_pushes_the_second_group_off_the_first_groups_token():
    """Step 0, beam 2 in 2 groups over 4 columns with p = (0.5, 0.3, 0.15, 0.05): group 0 takes column 0.  Group 1
    ranks column 0 at log 0.5 - lambda: above log 0.3 = -1.204 for lambda = 0.3 (-0.993), below for lambda = 1
    (-1.693), so group 1 moves to column 1."""
    logp = torch.tensor([0.5, 0.3, 0.15, 0.05]).log()
    lp = lp_table(0.0, 4)
    start = [dict(seq=[], score=0.0, fin=False, L=0)] * 2
    for lam, want in ((0.0, 0), (0.3, 0), (1.0, 1)):
        new = diverse_step(start, {0: logp, 1: logp}, 0, 2, lam, lp, end=3)
        assert [h["seq"] for h in new] == [[0], [want]], lam
        assert new[1]["score"] == float(logp[want])            # the raw log-probability, not the penalised key
    # one step later: group 0 expanded column 2, so group 1's column 2 pays one lambda, column 1 none
    hyps = [dict(seq=[0], score=-1.0, fin=False, L=1), dict(seq=[1], score=-1.0, fin=False, L=1)]
    row = torch.tensor([0.05, 0.3, 0.6, 0.05]).log()
    new = diverse_step(hyps, {0: row, 1: row}, 1, 2, 1.0, lp, end=3)
    assert [h["seq"] for h in new] == [[0, 2], [1, 1]]
    # an ended hypothesis competes as it is and its column counts for no one
    hyps = [dict(seq=[3], score=-0.1, fin=True, L=1), dict(seq=[3], score=-0.1, fin=True, L=1)]
    new = diverse_step(hyps, {}, 1, 2, 5.0, lp, end=3)
    assert [h["seq"] for h in new] == [[3], [3]] and all(h["fin"] for h in new)


def test_large_penalty_spreads_the_first_tokens():
    """G = beam, lambda = 1e4: at step 0 the groups take the G best first tokens, in order."""
    cfg, P, ents, facts, enc = case("geo")
    _, _, _, groups = predict_diverse_beam(cfg, P, enc, 1, ents, facts, 4, 4, 1e4)
    first = [g[0][0][0] for g in groups]
    with torch.no_grad():
        ee = R.entity_encode(cfg, P, ents, facts)
        mem = R.build_memory(cfg, P, enc, ee, None)
        logp = step_logp(cfg, P, ee, None, mem, R.pe_table(1, cfg.emb_dim).unsqueeze(0), facts, ents.shape[1], [], 0, 1)
    assert first == logp.topk(4).indices.tolist()
    assert group_best([(None, 0, 1, -2.0), (None, 0, 1, -1.0), (None, 0, 1, -1.0)]) == 1


def test_diversity_layout_matches_header(built_lib):
    import ick_amd.lib as L
    src = '#include <stdio.h>\n#include "ick_amd.h"\nint main(){printf("%zu", sizeof(ick_decode_diversity));}\n'
    with tempfile.TemporaryDirectory() as td:
        c = os.path.join(td, "sz.c")
        open(c, "w").write(src)
        exe = os.path.join(td, "sz")
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
        size = int(subprocess.check_output([exe]))
    assert ctypes.sizeof(L.DecodeDiversity) == size == 16


def test_library_exports_the_diverse_symbol(built_lib):
    import ick_amd.lib as L
    lib = ctypes.CDLL(built_lib)
    s = "ick_decode_select_beam_diverse"
    assert hasattr(lib, s) and s in L.SIGNATURES and len(L.SIGNATURES[s]) == 6


def test_one_group_keeps_the_defaults_signature():
    """G = 1 takes the calls without groups: the defaults are 1 and 0.0, and return_groups is off."""
    import inspect
    import ick_amd.decoder as D
    sig = inspect.signature(D.DecoderTransformer.predict_beam)
    assert sig.parameters["num_beam_groups"].default == 1
    assert sig.parameters["diversity_penalty"].default == 0.0 and sig.parameters["return_groups"].default is False
    assert D.check_diversity("x", 5) is False and D.check_diversity("x", 6, 3, 0.0) is True
