"""CPU checks of constrained beam search (predict_beam(force_tokens)): argument errors, a bank
allocation worked by hand, the CPU reference with every slot empty against the rules beam search, the closed <end>,
slots that share an id, and the ABI of the new entry point."""
import ctypes
import inspect
import os
import subprocess
import tempfile

import pytest
import torch

import ick_amd
import ick_amd.synth as synth
from ick_amd.lib import IckError
from oracle import restatement as R
from beam_rules_ref import lp_table, predict_beam_rules
from constrained_beam_ref import allocate, best_slot, constrained_step, predict_constrained_beam, slots_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
V, K = 50, 5                    # the argument-error decoder: columns 0 .. V + K - 1


@pytest.fixture(scope="module")
def built_lib():
    import ick_amd.build as build
    return build.build()


def cpu_decoder(variant="geo", V=V):
    m = ick_amd.load_models(variant)
    return m.DecoderTransformer(word_map=synth.make_word_map(V), emb_dim=300, decoder_dim=512, encoder_dim=512,
                                num_heads=10, num_layers=3)


WM = synth.make_word_map(V)
# (beam_size, keyword arguments) for a batch of one
BAD = [(4, dict(force_tokens=torch.tensor([3, 4]))),                              # not (B, C)
       (4, dict(force_tokens=torch.zeros(1, 0, dtype=torch.long))),               # C = 0
       (4, dict(force_tokens=torch.full((1, 9), 3))),                             # C = 9
       (4, dict(force_tokens=torch.full((2, 2), 3))),                             # B = 2 for one caption
       (4, dict(force_tokens=torch.tensor([[3.0, 4.0]]))),                        # not integers
       (4, dict(force_tokens=torch.tensor([[True, False]]))),
       (4, dict(force_tokens=[[3.5]])),
       (4, dict(force_tokens="3")),
       (4, dict(force_tokens=[[3], [4, 5]])),                                     # ragged
       (4, dict(force_tokens=[[-2]])),
       (4, dict(force_tokens=[[V + K]])),                                         # one past the last entity column
       (4, dict(force_tokens=[[3, WM["<start>"]]])),
       (4, dict(force_tokens=[[WM["<end>"]]])),
       (4, dict(force_tokens=torch.tensor([[3, WM["<pad>"]]], dtype=torch.int32))),
       (4, dict(force_tokens=[[3]], num_beam_groups=2, diversity_penalty=0.5)),
       (1, dict(force_tokens=[[V + K]]))]


@pytest.mark.parametrize("beam,kw", BAD, ids=lambda x: repr(x).replace("\n", "") if isinstance(x, dict) else "b%d" % x)
def test_argument_errors(beam, kw):
    """Every one raises IckError before any device work (this decoder has no GPU copy of anything)."""
    dec = cpu_decoder()
    enc = torch.zeros(1, 512, 14, 14)
    ents = synth.make_entities("geo", 1, K, V, 1)
    with pytest.raises(IckError):
        dec.predict_beam(enc, 12, ents, beam_size=beam, **kw)


def test_check_force_pads_to_eight_slots():
    import ick_amd.decoder as D
    special = [WM[w] for w in ("<start>", "<end>", "<pad>")]
    assert D.check_force("x", 2, V + K, special) is None
    out = D.check_force("x", 2, V + K, special, [[3, -1, V + 2], [-1, -1, -1]])
    assert out.dtype == torch.int32 and out.tolist() == [[3, -1, V + 2, -1, -1, -1, -1, -1], [-1] * 8]
    out = D.check_force("x", 1, V + K, special, torch.arange(3, 11, dtype=torch.int16).view(1, 8))
    assert out.tolist() == [list(range(3, 11))]


def test_force_tokens_defaults_to_none():
    import ick_amd.decoder as D
    assert inspect.signature(D.DecoderTransformer.predict_beam).parameters["force_tokens"].default is None


# ------------------------------------------------------------------------------------------------ by hand
def start(beam):
    return [dict(seq=[], score=0.0, fin=False, L=0, met=0)] + [None] * (beam - 1)


def test_bank_allocation_by_hand():
    """5 columns, <end> = 4, slots (2, 3), beam 3.
    Step 0, p = (.4, .3, .15, .1, .05): columns 0, 1 make bank 0, columns 2, 3 bank 1, <end> is closed.  Visits: bank 2
    is empty, bank 1 gives column 2, bank 0 column 0, round again, bank 1 gives column 3: [2], [0], [3], where the plain
    top 3 is [0], [1], [2].
    Step 1, rows 0 and 1 with the same p, row 2 with (.3, .3, .2, .15, .05): bank 2 holds row 2 + column 2 (.1 x .2 =
    .02) and row 0 + column 3 (.15 x .1 = .015); bank 1's best are row 0 + column 0 and row 1 + column 2, the same
    fp32 sum of the same two logs, so the lower row wins; bank 0's best is row 1 + column 0 (.16).  Three visits:
    [3, 2], [2, 0], [0, 0]; the plain top 3 would be .16, .12 and a .06."""
    lp = lp_table(0.0, 4)
    force = [2, 3]
    p = torch.tensor([0.4, 0.3, 0.15, 0.1, 0.05]).log()
    new = constrained_step(start(3), {0: p}, 0, force, lp, end=4)
    assert [h["seq"] for h in new] == [[2], [0], [3]]
    assert [h["met"] for h in new] == [1, 0, 2]
    assert p.topk(3).indices.tolist() == [0, 1, 2]                       # what the plain search keeps
    assert [h["score"] for h in new] == [float(p[2]), float(p[0]), float(p[3])]
    p2 = torch.tensor([0.3, 0.3, 0.2, 0.15, 0.05]).log()
    new2 = constrained_step(new, {0: p, 1: p, 2: p2}, 1, force, lp, end=4)
    assert [h["seq"] for h in new2] == [[3, 2], [2, 0], [0, 0]]
    assert [h["met"] for h in new2] == [3, 1, 0]
    plain = sorted(((h["score"] + float(r[w]), j, w) for j, (h, r) in enumerate(zip(new, (p, p, p2)))
                    for w in range(5)), key=lambda c: (-c[0], c[1], c[2]))[:3]
    assert [(j, w) for _, j, w in plain] == [(1, 0), (1, 1), (0, 0)]
    # the best is the best of the highest bank, not the best key
    assert best_slot(new2, lp) == 0 and new2[0]["score"] < new2[2]["score"]


def test_allocate_visits_banks_round_robin():
    c = [(-1.0, 0, 0, 2), (-2.0, 0, 1, 2), (-0.1, 1, 0, 0), (-0.2, 1, 1, 0), (-0.3, 1, 2, 0)]
    assert [x[:3] for x in allocate(c, 2, 4)] == [(-1.0, 0, 0), (-0.1, 1, 0), (-2.0, 0, 1), (-0.2, 1, 1)]
    assert [x[:3] for x in allocate(c, 3, 5)] == [(-1.0, 0, 0), (-0.1, 1, 0), (-2.0, 0, 1), (-0.2, 1, 1), (-0.3, 1, 2)]
    assert [x[:3] for x in allocate(c[2:], 0, 2)] == [(-0.1, 1, 0), (-0.2, 1, 1)]        # one bank: the plain top k
    assert len(allocate(c[:1], 2, 3)) == 1                                               # fewer candidates than slots


def test_end_stays_closed_until_every_slot_is_met():
    """<end> = 4 has p = .9 in every row.  A hypothesis with an unmet slot cannot take it; one that has met both takes
    it at once."""
    lp = lp_table(0.0, 6)
    force = [2, 3, -1]
    p = torch.tensor([0.03, 0.03, 0.02, 0.02, 0.9]).log()
    hyps = start(3)
    for i in range(2):
        hyps = constrained_step(hyps, {j: p for j, h in enumerate(hyps) if h is not None}, i, force, lp, end=4)
        assert all(not h["fin"] and 4 not in h["seq"] for h in hyps if h is not None), i
    assert hyps[0]["met"] == 3 and sorted(hyps[0]["seq"]) == [2, 3]
    hyps = constrained_step(hyps, {j: p for j, h in enumerate(hyps) if h is not None}, 2, force, lp, end=4)
    assert hyps[0]["seq"][-1] == 4 and hyps[0]["fin"] and hyps[0]["met"] == 3
    assert all(h["met"] == 3 for h in hyps if h["fin"])
    # an ended hypothesis competes as it is, with its bank
    again = constrained_step(hyps, {j: p for j, h in enumerate(hyps) if not h["fin"]}, 3, force, lp, end=4)
    assert again[0]["seq"] == hyps[0]["seq"] and again[0]["score"] == hyps[0]["score"]


def test_slots_with_the_same_id_are_met_together():
    lp = lp_table(0.0, 4)
    force = [2, -1, 2, 1]
    assert slots_of(force, 2) == 0b101 and slots_of(force, 1) == 0b1000 and slots_of(force, 0) == 0
    p = torch.tensor([0.4, 0.3, 0.15, 0.1, 0.05]).log()
    new = constrained_step(start(2), {0: p}, 0, force, lp, end=4)
    # n_req = 3: column 2 fills two slots at once (bank 2), column 1 one (bank 1)
    assert [(h["seq"], h["met"]) for h in new] == [([2], 0b101), ([1], 0b1000)]
    new = constrained_step(new, {0: p, 1: p}, 1, force, lp, end=4)
    assert (new[0]["seq"], new[0]["met"]) == ([2, 1], 0b1101)


# ------------------------------------------------------------------------------------------------ on the oracle
def case(variant, V=50, K=5, Fn=4, seed=3):
    cfg = R.config_from_word_map(variant, synth.make_word_map(V))
    P = synth.make_params(variant, V, seed)
    ents = synth.make_entities(variant, 1, K, V, seed)
    facts = synth.make_facts(variant, 1, Fn, K, seed) if variant != "geo" else None
    return cfg, P, ents, facts, synth.make_enc_out(1, seed)


@pytest.mark.parametrize("variant,beam,rules", [("geo", 3, True), ("knowledge", 2, False), ("geo", 4, False)])
def test_all_slots_empty_is_the_rules_beam(variant, beam, rules):
    cfg, P, ents, facts, enc = case(variant)
    kw = dict(length_penalty=0.6, no_repeat_ngram_size=2, min_len=3) if rules else {}
    ref = predict_beam_rules(cfg, P, enc, 7, ents, facts, beam, **kw)
    for force in ((), (-1, -1, -1)):
        mine = predict_constrained_beam(cfg, P, enc, 7, ents, facts, beam, force, **kw)
        assert torch.equal(mine[0], ref[0]) and mine[1] == ref[1] and mine[2] == ref[2] and mine[3] == 0
        assert [h[:3] for h in mine[4]] == [tuple(h) for h in ref[3]]


@pytest.mark.parametrize("variant,rules", [("geo", True), ("knowledge", False)])
def test_reference_keeps_the_promise(variant, rules):
    """Entity and fact pointers the plain search does not emit are all in the constrained best, and every ended
    hypothesis has them."""
    cfg, P, ents, facts, enc = case(variant)
    Vx = 50 + 5 + (4 if variant != "geo" else 0)
    kw = dict(length_penalty=0.6, no_repeat_ngram_size=2, min_len=3) if rules else {}
    plain = predict_beam_rules(cfg, P, enc, 8, ents, facts, 3, **kw)[0].tolist()
    force = [w for w in (Vx - 1, 52, 7, 50) if w not in plain][:3]
    assert len(force) == 3
    seq, score, _, bank, slots = predict_constrained_beam(cfg, P, enc, 8, ents, facts, 3, force, **kw)
    assert bank == 3 and all(w in seq.tolist() for w in force)
    for h in slots:
        if h is not None and h[0][-1] == cfg.end:
            assert all(w in h[0] for w in force)


# ------------------------------------------------------------------------------------------------ ABI
def test_constraints_layout_matches_header(built_lib):
    import ick_amd.lib as L
    src = '#include <stdio.h>\n#include "ick_amd.h"\nint main(){printf("%zu", sizeof(ick_decode_constraints));}\n'
    with tempfile.TemporaryDirectory() as td:
        c = os.path.join(td, "sz.c")
        open(c, "w").write(src)
        exe = os.path.join(td, "sz")
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
        size = int(subprocess.check_output([exe]))
    assert ctypes.sizeof(L.DecodeConstraints) == size == 16


def test_library_exports_the_forced_symbol(built_lib):
    import ick_amd.lib as L
    import ick_amd.ops as ops
    lib = ctypes.CDLL(built_lib)
    s = "ick_decode_select_beam_forced"
    assert hasattr(lib, s) and s in L.SIGNATURES and len(L.SIGNATURES[s]) == 6
    assert callable(ops.decode_select_beam_forced)
