"""Caption scoring on the MI355X: ick_row_logprob_rank / ick_caption_score_sums alone against tests/score_ref.py, and
DecoderTransformer.score_captions / score_tokens / train.validate(val_token_metrics) against the fp64 CPU oracle.

Bars (tests/test_decode_envelope_gpu.py): scores within TOL = 2e-4 of fp64, LP_TOL = 1e-4 per token log-probability,
SEQ_TOL = 1e-3 per caption sum.  A device rank is never compared for equality with the oracle's (another column lies
within 1e-4 of the target's score in many rows): it must lie in [#{s_j > s_t + eps}, #{s_j >= s_t - eps} - 1] of the
fp64 scores with eps = 2 * TOL (both scores may move by TOL), for every row.  On the kernel-alone matrices the values
are multiples of 1/8, so rank and argmax are exact."""
import functools

import numpy as np
import pytest
import torch

import ick_amd
import ick_amd.ops as ops
import ick_amd.synth as synth
from decode_ref import float64_default, params64
from oracle import restatement as R
from score_ref import score_batch

pytestmark = pytest.mark.gpu

TOL, SEQ_TOL, LP_TOL = 2e-4, 1e-3, 1e-4
EPS = 2 * TOL
SENT = (7.5, -7, -7)          # sentinel values of (token_log_probs, rank, best) no launch writes


# ------------------------------------------------------------------------------------------------ helpers
def pack_of(lengths, R_, L, count=None):
    pack = ops.HeadRows(torch.tensor(lengths, dtype=torch.int64, device="cuda"), R_, L)
    if count is not None:               # a hand-made row count (the kernel reads it from the device)
        pack.count = torch.tensor([count], dtype=torch.int32, device="cuda")
    return pack


def sentinel_out(R_, T):
    return (torch.full((R_, T), SENT[0], device="cuda"), torch.full((R_, T), SENT[1], dtype=torch.int32, device="cuda"),
            torch.full((R_, T), SENT[2], dtype=torch.int32, device="cuda"))


def logical_rows(lengths, L):
    """[(b, t)] of the packed rows, in ick_head_rowmap's order."""
    return [(b, t) for b, n in enumerate(lengths) for t in range(min(L - 1, max(0, n - 1)))]


def eighths(gen, *shape):
    return torch.randint(-32, 33, shape, generator=gen).float() / 8


# ------------------------------------------------------------------------------------------------ 1. the kernel alone
LAYOUTS = ("tight", "padded", "offset")


def kernel_case(Vx, layout):
    """Packed score rows for 2 captions of lengths (5, 7) at L = 7 (10 rows), with planted targets.  Where V+K+F is a
    multiple of 4 (256, 10 020) the aligned layouts have no scalar tail and the "tail" target is column Vx - 2; the sizes
    53, 1027 and 50 071 put it inside the tail.  At Vx = 1 every in-range target is column 0: that size is there for the
    one-column row, not for the planted columns."""
    R_, L, lengths = 2, 7, [5, 7]
    rows = logical_rows(lengths, L)
    gen = torch.Generator().manual_seed(Vx)
    ld = Vx if layout == "tight" else (Vx + 3) // 4 * 4
    off = 1 if layout == "offset" else 0
    packed = eighths(gen, R_ * L, Vx)
    pad = 2 if Vx > 2 else 7
    tail = 4 * (Vx // 4) if Vx % 4 else max(0, Vx - 2)
    tie, tie2 = Vx // 2, min(Vx - 1, Vx // 3 + 1)
    rnd = torch.randint(0, Vx, (2,), generator=gen).tolist()
    targets = [0, Vx - 1, min(tail, Vx - 1), tie, pad, Vx, -1, rnd[0], rnd[1], tie2]
    if tie != pad:
        packed[3, tie] = 4.0                      # the target holds the row's maximum ...
        packed[3, min(Vx - 1, tie + 5)] = 4.0     # ... and so does a later column (and, at random, earlier ones)
    packed[9, :] = 1.25                           # a row of one value: rank = the target's column, argmax = column 0
    caps = torch.zeros(R_, L, dtype=torch.int64)
    for m, (b, t) in enumerate(rows):
        caps[b, t + 1] = targets[m]
    buf = torch.zeros(R_ * L * ld + 4, device="cuda")
    scores = buf[off:off + R_ * L * ld].view(R_, L, ld)[:, :, :Vx]
    scores.copy_(packed.view(R_, L, Vx))
    logical = np.zeros((R_, L, Vx), np.float32)
    for m, (b, t) in enumerate(rows):
        logical[b, t] = packed[m].numpy()
    return R_, L, lengths, rows, scores, caps, pad, logical


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("Vx", [1, 53, 256, 1027, 10020, 50071])
def test_row_kernel_exact_on_eighths(Vx, layout):
    R_, L, lengths, rows, scores, caps, pad, logical = kernel_case(Vx, layout)
    assert (scores.data_ptr() % 16 == 0) == (layout != "offset")
    ref = score_batch(logical, caps.numpy(), lengths, pad)
    capd = caps.cuda()
    for count in (len(rows), 6, 0):           # the whole list, fewer rows than the grid holds, none
        out = sentinel_out(R_, L - 1)
        ops.row_logprob_rank(scores, capd, pack_of(lengths, R_, L, count), pad, out=out)
        tlp, rank, best = (x.cpu().numpy() for x in out)
        written = np.zeros((R_, L - 1), bool)
        worst = 0.0
        for m, (b, t) in enumerate(rows[:count]):
            written[b, t] = True
            assert rank[b, t] == ref["rank"][b, t] and best[b, t] == ref["best"][b, t], (Vx, layout, m)
            worst = max(worst, abs(tlp[b, t] - ref["token_log_probs"][b, t]))
        print("Vx %d %s count %d: max |lp - ref| %.2e" % (Vx, layout, count, worst))
        assert worst < LP_TOL, (Vx, layout)
        # rows at or past the count, and positions that are no row at all, keep the sentinels
        assert (tlp[~written] == SENT[0]).all() and (rank[~written] == SENT[1]).all() and (best[~written] == SENT[2]).all()
    # the planted rows did what they were planted for
    inval = [rows[m] for m in (4, 5, 6)]
    assert all(ref["rank"][b, t] == -1 for b, t in inval)
    b9, t9 = rows[9]
    assert ref["best"][b9, t9] == 0 and ref["rank"][b9, t9] == int(caps[b9, t9 + 1])
    if Vx > 8:
        b3, t3 = rows[3]
        assert ref["best"][b3, t3] <= Vx // 2 and ref["rank"][b3, t3] <= Vx // 2


# ------------------------------------------------------------------------------------------------ 2. sums and totals
@pytest.mark.parametrize("L,lengths", [(6, [1, 2, 6, 9, 4]), (2, [1, 2, 5]), (5, [4]), (4, [1, 1, 1]), (6, [6, 6])],
                         ids=["mixed", "L2", "B1", "all_length_1", "pad_inside"])
def test_caption_sums_and_totals(L, lengths):
    R_, Vx, pad, top_k = len(lengths), 53, 0, 3
    gen = torch.Generator().manual_seed(L * 100 + R_)
    rows = logical_rows(lengths, L)
    packed = eighths(gen, R_ * L, Vx)
    caps = torch.randint(1, Vx, (R_, L), generator=gen)
    if lengths == [6, 6]:
        caps[0, 3] = pad              # a <pad> target inside a caption is not scored
        caps[1, 2] = Vx + 4           # nor is a column outside the row
    logical = np.zeros((R_, L, Vx), np.float32)
    for m, (b, t) in enumerate(rows):
        logical[b, t] = packed[m].numpy()
    ref = score_batch(logical, caps.numpy(), lengths, pad, top_k=top_k)
    pack = pack_of(lengths, R_, L)
    assert int(pack.count.item()) == len(rows)
    out = sentinel_out(R_, L - 1)
    ops.row_logprob_rank(packed.view(R_, L, Vx).cuda(), caps.cuda(), pack, pad, out=out)
    res = ops.caption_score_sums(pack, *out, top_k=top_k)
    tlp, rank, best = (x.cpu().numpy() for x in out)
    log_prob, tokens, loss_sum, count, top1, topk = (x.cpu().numpy() for x in res)
    assert np.array_equal(rank, ref["rank"]) and np.array_equal(best, ref["best"])      # fills included: -1 / -1
    assert (tlp[rank < 0] == 0).all() and np.abs(tlp - ref["token_log_probs"]).max(initial=0) < LP_TOL
    assert np.array_equal(tokens, ref["tokens"]) and np.abs(log_prob - ref["log_prob"]).max() < SEQ_TOL
    assert count[0] == ref["count"] and top1[0] == ref["top1_hits"] and topk[0] == ref["topk_hits"]
    assert abs(loss_sum[0] - ref["loss_sum"]) < LP_TOL * max(1, ref["count"])
    if len(rows) == 0:
        assert count[0] == 0 and loss_sum[0] == 0 and (log_prob == 0).all() and (tokens == 0).all()
    # position order: the device sum is the float32 sum of its own token values, left to right
    for r in range(R_):
        s = np.float32(0)
        for t in range(L - 1):
            if rank[r, t] >= 0:
                s = np.float32(s + tlp[r, t])
        assert s == log_prob[r]


# ------------------------------------------------------------------------------------------------ 3. end to end
E2E = {"geo": dict(variant="geo", B=6, L=12, K=6, V=1000, F=0, seed=3),
       "knowledge": dict(variant="knowledge", B=6, L=12, K=6, V=500, F=5, seed=4),
       "news": dict(variant="news", B=6, L=12, K=6, V=300, F=5, seed=5),
       "geo_V49200": dict(variant="geo", B=3, L=8, K=20, V=49200, F=0, seed=6)}


def build_decoder(variant, V, P, wm=None):
    m = ick_amd.load_models(variant)
    dec = m.DecoderTransformer(word_map=wm or synth.make_word_map(V), emb_dim=300, decoder_dim=512, encoder_dim=512,
                               num_heads=10, num_layers=3)
    missing, unexpected = dec.load_state_dict(P, strict=False)
    assert missing == ["pos_encoder.pe"] and not unexpected
    return dec.cuda().eval()


def oracle_scores64(cfg, P, batch, enc):
    """R.forward in float64, un-sorted back to the input order: (B, L, Vx) numpy."""
    with torch.no_grad(), float64_default():
        st = {}
        s, _, _ = R.forward(cfg, params64(P), batch["captions"], enc.double(), batch["caption_masks"],
                            batch["caption_lengths"], batch["entities"].double(), batch.get("facts"), stages=st)
    out = torch.empty_like(s)
    out[st["sort_ind"]] = s
    return out.numpy()


@functools.lru_cache(maxsize=None)
def e2e_case(name):
    c = E2E[name]
    P = synth.make_params(c["variant"], c["V"], c["seed"])
    cfg = R.config_from_word_map(c["variant"], synth.make_word_map(c["V"]))
    batch = synth.make_batch(c["variant"], c["B"], c["L"], c["K"], c["V"], c["F"], c["seed"])
    enc = synth.make_enc_out(c["B"], c["seed"])
    s64 = oracle_scores64(cfg, P, batch, enc)
    ref = score_batch(s64, batch["captions"].numpy(), batch["caption_lengths"].view(-1).tolist(), cfg.pad, eps=EPS)
    return c, cfg, P, batch, enc, ref


def call_score(dec, batch, enc, **kw):
    return dec.score_captions(batch["captions"].cuda(), enc.cuda(), batch["caption_masks"].cuda(),
                              batch["caption_lengths"].cuda(), batch["entities"],
                              batch["facts"].cuda() if "facts" in batch else None, **kw)


def check_against_oracle(got, ref, what, top_k=5):
    tlp, rank, best = got.token_log_probs.cpu().numpy(), got.rank.cpu().numpy(), got.best.cpu().numpy()
    ok = ref["rank"] >= 0
    assert np.array_equal(rank >= 0, ok), what
    assert (tlp[~ok] == 0).all() and (rank[~ok] == -1).all() and (best[~ok] == -1).all(), what
    err = np.abs(tlp - ref["token_log_probs"]).max()
    seq = np.abs(got.log_prob.cpu().numpy() - ref["log_prob"]).max()
    print("%s: max |token lp - fp64| %.2e, max |caption lp - fp64| %.2e, rows with a rank interval wider than one: %d of %d"
          % (what, err, seq, int((ref["hi"] > ref["lo"])[ok].sum()), int(ok.sum())))
    assert err < LP_TOL and seq < SEQ_TOL, what
    assert (ref["lo"][ok] <= rank[ok]).all() and (rank[ok] <= ref["hi"][ok]).all(), what          # every row
    clear = ok & (ref["margin"] > EPS)
    assert clear.any() and np.array_equal(best[clear], ref["best"][clear]), what
    assert np.array_equal(got.tokens.cpu().numpy(), ref["tokens"]) and got.count.item() == ref["count"], what
    assert abs(got.loss_sum.item() - ref["loss_sum"]) < LP_TOL * ref["count"], what
    lo1, hi1 = int((ref["hi"][ok] == 0).sum()), int((ref["lo"][ok] == 0).sum())
    lok, hik = int((ref["hi"][ok] < top_k).sum()), int((ref["lo"][ok] < top_k).sum())
    assert lo1 <= got.top1_hits.item() <= hi1 and lok <= got.topk_hits.item() <= hik, what
    assert got.top1_hits.item() == (rank[ok] == 0).sum() and got.topk_hits.item() == (rank[ok] < top_k).sum(), what


@pytest.mark.parametrize("name", list(E2E))
def test_score_captions_vs_oracle(name, gemm_split):
    c, cfg, P, batch, enc, ref = e2e_case(name)
    dec = build_decoder(c["variant"], c["V"], P)
    got = call_score(dec, batch, enc)
    T = c["L"] - 1
    assert got.token_log_probs.shape == got.rank.shape == got.best.shape == (c["B"], T)
    assert got.log_prob.shape == got.tokens.shape == (c["B"],) and got.rank.dtype == got.tokens.dtype == torch.int32
    assert all(x.shape == (1,) and x.dtype == torch.float32 for x in (got.loss_sum, got.count, got.top1_hits, got.topk_hits))
    check_against_oracle(got, ref, "%s (split mode %d)" % (name, gemm_split))


# ------------------------------------------------------------------------------------------------ 4. image_index
def fields(s):
    return (s.log_prob, s.tokens, s.token_log_probs, s.rank, s.best, s.loss_sum, s.count, s.top1_hits, s.topk_hits)


def index_case():
    variant, B, R_, L, K, V, seed = "geo", 3, 7, 10, 6, 400, 8
    P = synth.make_params(variant, V, seed)
    caps, masks, lens = synth.make_captions(variant, R_, L, K, 0, V, seed)
    ents = synth.make_entities(variant, B, K, V, seed)
    enc = synth.make_enc_out(B, seed)
    idx = torch.tensor([0, 0, 1, 1, 1, 2, 2])
    return build_decoder(variant, V, P), caps.cuda(), masks.cuda(), lens.cuda(), ents, enc.cuda(), idx


def test_image_index_equals_repeated_rows():
    dec, caps, masks, lens, ents, enc, idx = index_case()
    for graphs in (False, True):
        dec.use_hip_graphs = graphs
        a = dec.score_captions(caps, enc, masks, lens, ents, image_index=idx.cuda())
        b = dec.score_captions(caps, enc[idx.cuda()], masks, lens, ents[idx])
        assert torch.equal(a.tokens, b.tokens) and torch.equal(a.count, b.count)
        if not graphs:
            assert all(torch.equal(x, y) for x, y in zip(fields(a), fields(b)))          # eager: bit for bit
        assert (a.token_log_probs - b.token_log_probs).abs().max().item() <= 1e-5
        assert (a.log_prob - b.log_prob).abs().max().item() <= 1e-5
        # the first two captions (both of image 0) scored alone
        c = dec.score_captions(caps[:2], enc[:1], masks[:2], lens[:2], ents[:1],
                               image_index=torch.zeros(2, dtype=torch.int64))
        assert (c.token_log_probs - a.token_log_probs[:2]).abs().max().item() <= 1e-5
        assert (c.log_prob - a.log_prob[:2]).abs().max().item() <= 1e-5 and torch.equal(c.tokens, a.tokens[:2])
    with pytest.raises(ick_amd.lib.IckError):
        dec.score_captions(caps, enc, masks, lens, ents, image_index=torch.tensor([0, 0, 1, 1, 1, 2, 3]))
    with pytest.raises(ick_amd.lib.IckError):
        dec.score_captions(caps, enc, masks, lens, ents)


# ------------------------------------------------------------------------------------------------ 5. replay
def test_replay_eager_and_dropout():
    c, cfg, P, batch, enc, ref = e2e_case("knowledge")
    dec = build_decoder(c["variant"], c["V"], P)
    first = call_score(dec, batch, enc)
    graphs = dict(dec.__dict__["_graphs"])
    assert len(graphs) == 1 and next(iter(graphs))[0] == "score"
    kept = [x.clone() for x in fields(first)]
    other = dict(batch)
    other["captions"], other["caption_masks"], other["caption_lengths"] = synth.make_captions(
        c["variant"], c["B"], c["L"], c["K"], c["F"], c["V"], c["seed"] + 1)
    second = call_score(dec, other, enc)                       # same shapes, new captions: a replay
    assert dict(dec.__dict__["_graphs"]).keys() == graphs.keys()
    assert not torch.equal(second.token_log_probs, first.token_log_probs)
    assert all(torch.equal(x, y) for x, y in zip(fields(first), kept))       # results are the caller's, not the graph's
    s64 = oracle_scores64(cfg, P, other, enc)
    check_against_oracle(second, score_batch(s64, other["captions"].numpy(), other["caption_lengths"].view(-1).tolist(),
                                             cfg.pad, eps=EPS), "replay with new captions")
    again = call_score(dec, batch, enc)
    assert all(torch.equal(x, y) for x, y in zip(fields(again), kept))       # two identical calls: bit-identical
    dec.use_hip_graphs = False
    eager = call_score(dec, batch, enc)
    assert all(torch.equal(x, y) for x, y in zip(fields(eager), kept))       # graphed == eager
    dec.use_hip_graphs = True
    dec.train()                                                              # dropout 0.5 / 0.1 in the module
    assert dec.transformer_decoder.layers[0].dropout.p > 0 and dec.training
    for graphs_on in (True, False):
        dec.use_hip_graphs = graphs_on
        tr = call_score(dec, batch, enc)
        assert all(torch.equal(x, y) for x, y in zip(fields(tr), kept))      # train() mode: the bits of eval()
        assert not any(x.requires_grad for x in fields(tr))


# ------------------------------------------------------------------------------------------------ 6. decode cross-check
def oracle_both_forms(cfg, P, enc, ents, facts, seqs, n, max_len):
    """CPU oracle, per decoded sequence: its log-probability under the teacher-forced forward (R.forward: the context
    indicators of position p see the mentions strictly before p -- get_context_indicators mode 0) and under the
    step-by-step form the decode kernels restate (R.sequence_logprob: the indicators see the whole buffer, the token
    being fed included -- mode 1).  -> (teacher forced (N,), step by step (N,))."""
    V, K = cfg.vocab_size, ents.shape[1]
    tf, sl = [], []
    with torch.no_grad():
        for r, seq in enumerate(seqs):
            b = r // n
            toks = []
            for q in seq:
                toks.append(int(q))
                if int(q) == cfg.end:
                    break
            caps = torch.tensor([[cfg.start] + toks + [cfg.pad] * (max_len - len(toks))])
            masks = torch.tensor([[0] + [2 if q >= V + K else (1 if q >= V else 0) for q in toks] +
                                  [0] * (max_len - len(toks))])       # predict()'s feedback rule
            f = None if facts is None else facts[b:b + 1]
            s, _, _ = R.forward(cfg, P, caps, enc[b:b + 1], masks, torch.tensor([[len(toks) + 1]]), ents[b:b + 1], f)
            tf.append(sum(float(s[0, t].log_softmax(-1)[toks[t]]) for t in range(len(toks))))
            sl.append(R.sequence_logprob(cfg, P, enc[b:b + 1], ents[b:b + 1], f, toks, max_len + 1))
    return torch.tensor(tf), torch.tensor(sl)


@pytest.mark.parametrize("variant", ["geo", "knowledge"])
def test_score_tokens_reproduces_decode_log_probs(variant):
    """score_tokens on decode output gives the decode's own log-probabilities back: per token for sampled rows, per
    hypothesis for a beam's.  Facts variants: the teacher-forced and the step-by-step context indicators differ at the
    step after an entity is first mentioned, so the CPU oracle scores every sequence in both forms
    first; where the two agree the cross-check is asserted as for geo, and where they do not, the device gap must be the
    oracle's gap -- each side stays within the single tolerance of its own oracle form."""
    B, K, V, F, max_len, n, beam, seed = 2, 6, 300, 5, 8, 2, 3, 9
    P = synth.make_params(variant, V, seed)
    cfg = R.config_from_word_map(variant, synth.make_word_map(V))
    dec = build_decoder(variant, V, P)
    ents = synth.make_entities(variant, B, K, V, seed)
    facts = synth.make_facts(variant, B, F, K, seed) if variant != "geo" else None
    enc = synth.make_enc_out(B, seed)
    fa = [] if facts is None else [facts.cuda()]
    toks, lps = dec.predict_sample(enc.cuda(), max_len, ents, *fa, num_samples=n, seed=3, return_log_probs=True)
    _, _, final, cum = dec.predict_beam(enc.cuda(), max_len, ents, *fa, beam_size=beam, return_all=True)
    hyps = final.reshape(-1, max_len)
    cum = cum.reshape(-1).cpu()
    assert torch.isfinite(cum).all()
    shift_s, shift_b = torch.zeros(B * n), torch.zeros(B * beam)        # oracle: teacher forced - step by step
    if variant != "geo":
        tf, sl = oracle_both_forms(cfg, P, enc, ents, facts, toks.t().cpu().tolist(), n, max_len)
        shift_s = tf - sl
        tf, sl = oracle_both_forms(cfg, P, enc, ents, facts, hyps.cpu().tolist(), beam, max_len)
        shift_b = tf - sl
        assert (sl - cum).abs().max().item() < SEQ_TOL                   # the beam's scores are the step-by-step form's
        print("%s: CPU oracle, teacher forced - step by step: samples max %.2e, beam hypotheses max %.2e"
              % (variant, shift_s.abs().max().item(), shift_b.abs().max().item()))
    s = dec.score_tokens(toks, enc.cuda(), ents, facts, samples_per_image=n)
    assert s.token_log_probs.shape == (B * n, max_len)
    live = (s.rank >= 0)
    is_end = (toks.t() == cfg.end).long()
    assert torch.equal(live, (torch.cumsum(is_end, 1) - is_end) == 0)          # up to and including the first <end>
    assert (s.token_log_probs[~live] == 0).all()
    agree = (shift_s.abs() < LP_TOL).cuda()
    assert agree.any(), "no sampled row on which the two oracle forms agree: the per-token check would be empty"
    gap = (s.token_log_probs - lps.t()).abs()[live & agree.view(-1, 1)].max().item()
    gaps = ((s.log_prob.cpu() - lps.sum(0).cpu()) - shift_s).abs().max().item()
    print("%s: score_tokens vs predict_sample: per token max gap %.2e (%d of %d rows), per row beside the oracle's %.2e"
          % (variant, gap, int(agree.sum()), B * n, gaps))
    assert gap < 2 * LP_TOL and gaps < 2 * SEQ_TOL
    sb = dec.score_tokens(hyps.t().contiguous(), enc.cuda(), ents, facts, samples_per_image=beam)
    gapb = ((sb.log_prob.cpu() - cum) - shift_b).abs().max().item()
    print("%s: score_tokens vs predict_beam hypothesis scores beside the oracle's gap: max %.2e" % (variant, gapb))
    assert gapb < 2 * SEQ_TOL
    if variant == "geo":
        assert agree.all()


# ------------------------------------------------------------------------------------------------ 7. validate
def test_validate_token_metrics(tmp_path, capsys):
    from ick_amd import train as tr
    variant, V, K, L = "geo", 60, 6, 12
    data_dir = str(tmp_path / "data")
    wm = synth.write_dataset(data_dir, "toy", variant, n_train=4, n_val=8, n_test=2, L=L, K=K, V=V, F=0)
    P = synth.make_params(variant, V, 1)
    dec = build_decoder(variant, V, P, wm)
    enc = ick_amd.load_models(variant).Encoder(emb_dim=300)
    cw, cb = synth.make_conv1(1)
    with torch.no_grad():
        enc.conv1.weight.copy_(cw)
        enc.conv1.bias.copy_(cb)
    enc = enc.cuda().eval()
    crit = torch.nn.CrossEntropyLoss(ignore_index=wm["<pad>"]).cuda()
    dev = torch.device("cuda")

    def run(flag):
        cfg = tr.Config(variant=variant, data_dir=data_dir, data_name="toy", batch_size=3, workers=0,
                        val_token_metrics=flag)
        loaders, _, _ = tr.make_loaders(cfg, 0, 1)
        capsys.readouterr()
        loss = tr.validate(loaders["VAL"], enc, dec, crit, cfg, dev)
        return loss, capsys.readouterr().out, loaders["VAL"]

    for k in ("val_perplexity", "val_top1", "val_top5"):
        tr.STATS.pop(k, None)
    off, printed, loader = run(False)
    assert printed == "" and not any(k.startswith("val_") for k in tr.STATS) and isinstance(off, float)
    assert run(False)[0] == off
    on, printed, _ = run(True)
    print("validate: loss off %.6f on %.6f" % (off, on))
    assert abs(on - off) < LP_TOL
    assert "perplexity" in printed and "top-1" in printed and "top-5" in printed
    assert abs(tr.STATS["val_perplexity"] - np.exp(on)) < 1e-9 * np.exp(on)
    # the oracle's rank intervals over the same batches bound the two accuracies
    cfg_o = R.config_from_word_map(variant, wm)
    lo1 = hi1 = lo5 = hi5 = cnt = 0
    for batch in loader:
        imgs, caps, lens, masks, ent = batch[0].float(), batch[1], batch[2], batch[3], batch[4]
        with torch.no_grad(), float64_default():
            e = R.feat_proj(imgs.double(), cw.double(), cb.double())
        b = dict(captions=caps, caption_masks=masks, caption_lengths=lens.view(-1, 1), entities=ent.float())
        ref = score_batch(oracle_scores64(cfg_o, P, b, e), caps.numpy(), lens.view(-1).tolist(), cfg_o.pad, eps=EPS)
        ok = ref["rank"] >= 0
        cnt += int(ok.sum())
        lo1 += int((ref["hi"][ok] == 0).sum()); hi1 += int((ref["lo"][ok] == 0).sum())
        lo5 += int((ref["hi"][ok] < 5).sum()); hi5 += int((ref["lo"][ok] < 5).sum())
    assert cnt > 0 and lo1 / cnt <= tr.STATS["val_top1"] <= hi1 / cnt and lo5 / cnt <= tr.STATS["val_top5"] <= hi5 / cnt
    assert tr.STATS["val_top1"] <= tr.STATS["val_top5"] <= 1.0
