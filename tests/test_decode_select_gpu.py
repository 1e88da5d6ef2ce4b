"""Greedy token selection of the fused decode (csrc/decode_select.hip: dec_select_kernel; csrc/decode.hip: fused_select,
the same selection folded into the next step's first launch).  Both, and ick_greedy_update (csrc/score_head.hip), take
predict()'s per-step decision from one function, greedy_step() (csrc/decode_select.h): the scripted test below drives
all three through every branch of it against the oracle's loop_cleanup (geo-aware/models.py:421-435)."""
import functools

import numpy as np
import pytest
import torch

import ick_amd.ops as ops
import ick_amd.synth as synth
from oracle import restatement as R
from decode_cases import Case
from test_decode_envelope_gpu import build
from test_forward_gpu import build_decoder

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------------ selection inside the step
@pytest.mark.parametrize("variant,B,K,V,Fn,max_len,seed", [("geo", 32, 20, 10000, 0, 20, 61), ("knowledge", 5, 9, 300, 11, 14, 4),
                                                           ("news", 3, 60, 90, 80, 7, 8), ("geo", 3, 6, 50, 0, 1, 2)])
def test_selection_folded_into_the_next_step_equals_selection_kernel(variant, B, K, V, Fn, max_len, seed):
    """predict() with the greedy selection inside the next step's first launch (11 launches per token) against the same
    decode with the selection kernel after every step: identical tokens, eager and replayed, at cfg5's size too.  (Both are
    pinned to the reference's predict() goldens by tests/test_forward_gpu.py, which runs the default = folded form.)"""
    P = synth.make_params(variant, V, seed)
    dec = build_decoder(variant, V, P)
    ents = synth.make_entities(variant, B, K, V, seed)
    facts = synth.make_facts(variant, B, Fn, K, seed).cuda() if variant != "geo" else None
    enc = synth.make_enc_out(B, seed).cuda()
    args = [enc, max_len, ents] + ([facts] if facts is not None else [])
    res = {}
    for fold in (False, True):
        for graphs in (False, True):
            dec.fuse_select, dec.use_hip_graphs = fold, graphs
            res[(fold, graphs)] = dec.predict(*args).clone()
            assert torch.equal(dec.predict(*args), res[(fold, graphs)])
    dec.fuse_select, dec.use_hip_graphs = True, True
    ref = res[(False, False)]
    assert ref.shape == (max_len, B)
    for k, v in res.items():
        assert torch.equal(v, ref), k


def test_selection_folded_cleanup_rules_vs_oracle(monkeypatch):
    """Seeds whose decode runs into predict()'s repeated n-gram clean-up (geo-aware/models.py:421-435): the folded
    selection keeps the last five outputs and three runner-ups in its window instead of reading the output array.
    A seed hits when the reference's own loop_cleanup rewrites its output: of seeds 0-7 that is 0, 2, 4, 6 (repeated
    token) and 3, 5 (repeated pair), counted on the CPU with R.predict alone."""
    variant, K, V, max_len = "geo", 6, 50, 12
    cfg = R.config_from_word_map(variant, synth.make_word_map(V))
    cleanups = []
    plain_cleanup = R.loop_cleanup

    def counting_cleanup(output, prev_top_two, i):
        before = list(output)
        plain_cleanup(output, prev_top_two, i)
        cleanups.append(output != before)

    monkeypatch.setattr(R, "loop_cleanup", counting_cleanup)
    hits = 0
    for seed in range(8):
        P = synth.make_params(variant, V, seed)
        dec = build_decoder(variant, V, P)
        ents = synth.make_entities(variant, 1, K, V, seed)
        enc = synth.make_enc_out(1, seed)
        del cleanups[:]
        with torch.no_grad():
            ref = R.predict(cfg, P, enc, max_len, ents)
        hits += any(cleanups)
        out = dec.predict(enc.cuda(), max_len, ents).cpu()
        assert out.view(-1).tolist() == ref.view(-1).tolist(), seed
    assert hits == 6


# ------------------------------------------------------------------------------------------------ scripted decisions
# The scripted (best, runner-up) streams of tests/test_ops_gpu.py::test_greedy_update_matches_reference_cleanup: a repeated
# token, pair and triple, pointer columns 52-54 and an <end>.
V, K, MAX_LEN, END = 50, 6, 14, 49
STREAMS = [
    [5, 5, 5, 7, 8, 7, 8, 9, 1, 2, 3, 1, 2, 3],
    [1, 2, 1, 2, 1, 2, 3, 3, 49, 4, 4, 4, 4, 4],
    [52, 52, 53, 54, 53, 54, 10, 11, 12, 10, 11, 12, 49, 1],
    [9, 8, 7, 6, 5, 4, 3, 2, 1, 9, 8, 7, 6, 5],
]
SEC = [[(t * 7 + b * 3 + 20) % 48 + 1 for t in range(MAX_LEN)] for b in range(len(STREAMS))]
NTILES, NONE = 2, 0x7fffffff                 # candidate tiles of 48 words (kVocabTile); index of an empty candidate slot


@functools.lru_cache(maxsize=None)
def scripted_reference():
    """(output, finished, fired) of the four streams by the oracle's loop (as test_greedy_update_matches_reference_cleanup
    runs it); fired counts the decisions: "end", and the n of the repeated n-gram loop_cleanup found (1, 2, 3)."""
    out = [[0] * MAX_LEN for _ in STREAMS]
    hist = [[] for _ in STREAMS]
    fin = [False] * len(STREAMS)
    fired = {"end": 0, 1: 0, 2: 0, 3: 0}
    for i in range(MAX_LEN):
        for b, s in enumerate(STREAMS):
            if fin[b]:
                continue
            out[b][i] = s[i]
            if s[i] == END:
                fin[b] = True
                fired["end"] += 1
                continue
            hist[b].append(SEC[b][i])
            # the repeat loop_cleanup is about to find: its own conditions, first match
            n = next((n for n in (1, 2, 3) if i > 2 * n - 2 and out[b][i - n + 1:i + 1] == out[b][i - 2 * n + 1:i - n + 1]), 0)
            before = list(out[b])
            R.loop_cleanup(out[b], hist[b], i)
            assert (out[b] != before) == (n != 0), (b, i)
            if n:
                fired[n] += 1
    return out, [int(f) for f in fin], fired


def step_buffers(R_, i):
    """The candidate tiles (R, NTILES, 4) = {value, index bits, value, index bits} and pointer scores (R, K) that make
    row r choose STREAMS[r % 4][i] with runner-up SEC[r % 4][i].  Words sit in the tile of their 48-word block, pointer
    columns (>= V) in the pointer scores; empty candidate slots are (-inf, NONE)."""
    val = np.full((R_, NTILES, 2), -np.inf, dtype=np.float32)
    idx = np.full((R_, NTILES, 2), NONE, dtype=np.int32)
    ptr = np.full((R_, K), -1e30, dtype=np.float32)
    for r in range(R_):
        b = r % len(STREAMS)
        for tok, v in ((STREAMS[b][i], 2.0), (SEC[b][i], 1.0)):       # best first: it takes a tile's first slot
            if tok >= V:
                ptr[r, tok - V] = v
            else:
                slot = int(idx[r, tok // 48, 0] != NONE)
                val[r, tok // 48, slot], idx[r, tok // 48, slot] = v, tok
    cand = np.stack([val[..., 0], idx[..., 0].view(np.float32), val[..., 1], idx[..., 1].view(np.float32)], axis=-1)
    return torch.from_numpy(cand.view(np.int32)).cuda(), torch.from_numpy(ptr).cuda()


def greedy_update_run(R_):
    """ops.greedy_update over the streams tiled to R rows: (output, finished, [(next_token, next_mask) after step i])."""
    output = torch.zeros(R_, MAX_LEN, dtype=torch.long, device="cuda")
    hist = torch.zeros(R_, MAX_LEN, dtype=torch.int32, device="cuda")
    fin = torch.zeros(R_, dtype=torch.int32, device="cuda")
    nt = torch.zeros(R_, dtype=torch.long, device="cuda")
    nm = torch.zeros(R_, dtype=torch.long, device="cuda")
    nxt = []
    for i in range(MAX_LEN):
        best = torch.tensor([STREAMS[r % 4][i] for r in range(R_)], dtype=torch.int32).cuda()
        second = torch.tensor([SEC[r % 4][i] for r in range(R_)], dtype=torch.int32).cuda()
        ops.greedy_update(best, second, output, hist, fin, nt, nm, i, V, K, False, END)
        nxt.append((nt.clone(), nm.clone()))
    return output, fin, nxt


@pytest.mark.parametrize("R_,g_self", [(5, 1), (33, 2), (67, 4), (131, 8)])
def test_scripted_selection_matches_reference_cleanup(R_, g_self):
    """dec_select_kernel at every step, and the folded sequence (fused_select<g_self> inside the first self block of the
    next step, dec_select_kernel once at the end), on hand-written candidate and pointer buffers: output and finished
    equal the oracle's loop and ick_greedy_update exactly, next_token / next_mask equal ick_greedy_update's after every
    step; the oracle alone says that <end> and each of the three clean-up branches fire in the streams.  (The last step
    has no next token: ick_greedy_update leaves a live row's as they were, the decode kernels write them, so there only
    the rows that have ended are compared.)  R covers every wave-to-row mapping of fused_select and a ragged last row
    group."""
    case = Case("scripted", "greedy", R_, layers=1, K=K, V=V, max_len=MAX_LEN)
    assert ops.decode_plan(R_, 1, case.d, case.H, case.FF)["g_self"] == g_self
    assert (case.d, case.H, case.FF) == (300, 10, 512)
    ref_out, ref_fin, fired = scripted_reference()
    assert all(n >= 1 for n in fired.values()), fired       # the reference alone: <end> and every clean-up branch fire
    assert ref_fin == [0, 1, 1, 0]      # two streams never end: the early exit on the finished count stays out of the way
    want_out = torch.tensor([ref_out[r % 4] for r in range(R_)])
    want_fin = torch.tensor([ref_fin[r % 4] for r in range(R_)], dtype=torch.int32)
    upd_out, upd_fin, upd_next = greedy_update_run(R_)
    assert torch.equal(upd_out.cpu(), want_out) and torch.equal(upd_fin.cpu(), want_fin)

    dec, _, _, ents, _, enc = build(case)
    assert dec.word_map["<end>"] == END and dec.word_map["<pad>"] == 0
    enc_out, ents, _ = dec._prepare_inputs(enc.cuda(), ents, None)
    enc_tok = dec._image_input(enc_out)[0].contiguous()
    ee, fe, kv, _, side = dec._encode_context(enc_tok, ents.contiguous(), None, None)
    side.join()
    bufs = [step_buffers(R_, i) for i in range(MAX_LEN)]

    def check_next(t, i, what):
        nt, nm = upd_next[i]
        rows = slice(None) if i < MAX_LEN - 1 else want_fin.cuda().bool()
        assert torch.equal(t["next_token"][rows], nt[rows]) and torch.equal(t["next_mask"][rows], nm[rows]), (what, i)

    for fold in (False, True):
        c, t = dec._decode_ctx(kv, ee, fe, 1, MAX_LEN, kv.shape[3], fuse_select=fold)
        cand = t["cand"].view(-1)[:R_ * NTILES * 4].view(torch.int32).view(R_, NTILES, 4)
        for i in range(MAX_LEN):
            if fold:
                ops.decode_layers_part(c, i, 1)       # i >= 1: the selection of step i - 1 inside the first self block
                if i >= 1:
                    check_next(t, i - 1, "folded")
            cand.copy_(bufs[i][0])
            t["ptr"].copy_(bufs[i][1])
            if not fold:
                ops.decode_select_greedy(c, i)
                check_next(t, i, "kernel")
        if fold:
            ops.decode_select_greedy(c, MAX_LEN - 1)
            check_next(t, MAX_LEN - 1, "folded")
        assert torch.equal(t["output"].cpu(), want_out), fold
        assert torch.equal(t["finished"].cpu(), want_fin), fold
