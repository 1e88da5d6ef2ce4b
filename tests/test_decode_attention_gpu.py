"""Cross-attention weights of greedy, beam and sampled decoding (return_attention, ick_decode_layers_attn) against the
float64 restatement of tests/attn_ref.py: every case of tests/decode_cases.py, every row, every live step, every layer
and head.  Also: the tokens, scores and log-probabilities do not change with return_attention; graph replays and
alternating calls are bit-identical; beam hypotheses get the weights of the rows that computed their positions."""
import numpy as np
import pytest
import torch

import ick_amd.decoder as D
import ick_amd.ops as ops
from ick_amd.lib import IckError
from attn_ref import cross_weights, prefix_feeds
from decode_cases import BY_NAME, CASES, Case
from decode_ref import Fp64Decode
from test_decode_envelope_gpu import args_of, build, check_plan

pytestmark = pytest.mark.gpu

ATOL, SUM_TOL = 5e-5, 1e-5


def greedy_production_attn(dec, enc, ents, facts, max_len):
    """predict()'s launch sequence with ick_decode_layers_attn, recording what each row was fed.  Returns (output (R,
    max_len), fed (R, max_len), raw weights (max_len, R, layers, H, S), before the zeroing after <end>)."""
    enc_out, ents, facts = dec._prepare_inputs(enc.cuda(), ents, None if facts is None else facts.cuda())
    enc_tok = dec._image_input(enc_out)[0].contiguous()
    K, V = ents.shape[1], dec.vocab_size
    ee, fe, kv, _, side = dec._encode_context(enc_tok, ents.contiguous(), facts, None)
    side.join()
    c, t = dec._decode_ctx(kv, ee, fe, 1, max_len, kv.shape[3], fuse_select=True)
    attn = torch.zeros(max_len, c.R, c.layers, c.H, c.S, device="cuda")
    fed = [torch.full((c.R,), dec.word_map["<start>"], dtype=torch.long, device="cuda")]
    for i in range(max_len):
        if i > 0:
            ops.decode_layers_attn(c, None, i, 1)       # attn=None: exactly ick_decode_layers_part
            fed.append(t["next_token"].clone())
        if dec.has_facts:
            ops.context_indicators(t["cap_buf"], facts, K, V, dec._pred_wt(), dec.fc_predicate.bias.detach(), mode=1,
                                   eib=t["eib"], gate=t["gate"])
        ops.decode_layers_attn(c, attn, i, 2 if i > 0 else 0)
    ops.decode_select_greedy(c, max_len - 1)
    torch.cuda.synchronize()
    return t["output"].cpu(), torch.stack(fed, dim=1).cpu(), attn.cpu()


def live_steps(out, end):
    return [(r.index(end) + 1 if end in r else len(r)) for r in out.tolist()]


def check_weights(name, got, ref, live):
    """got (max_len, R, layers, H, S) float32 tensor, ref (R, n, layers, H, S) fp64, live steps per row: fp64 within
    ATOL, every distribution sums to 1, exact zeros after the live steps.  Returns the worst error."""
    got = got.double().numpy()
    worst = 0.0
    for r, n in enumerate(live):
        g = got[:n, r]
        worst = max(worst, float(np.abs(g - ref[r, :n]).max()))
        assert np.abs(g.sum(-1) - 1.0).max() < SUM_TOL, (name, r)
        assert (got[n:, r] == 0).all(), (name, r, "not zero after <end>")
    assert worst < ATOL, (name, "max |weight - fp64|", worst)
    return worst


def run_case(case):
    check_plan(case)
    dec, cfg, P, ents, facts, enc = build(case)
    a = args_of(enc, ents, facts)
    fp64 = Fp64Decode(cfg, P, enc, ents, facts)
    if case.kind == "greedy":
        plain = dec.predict(a[0], case.max_len, *a[1:])
        seq, attn = dec.predict(a[0], case.max_len, *a[1:], return_attention=True)
        assert torch.equal(seq, plain), case.name
        assert attn.shape == (case.max_len, case.B, case.layers, case.H, case.S) and attn.dtype == torch.float32
        out, fed, raw = greedy_production_attn(dec, enc, ents, facts, case.max_len)
        assert torch.equal(out, seq.t().cpu()), case.name
        live = live_steps(out, cfg.end)
        ref = cross_weights(fp64, fed, torch.arange(case.B))
        worst = check_weights(case.name, attn.cpu(), ref, live)
        # the product path is the driven sequence, zeroed after <end>
        assert torch.equal(attn.cpu(), D._zero_after_end(raw, out, cfg.end)), case.name
    elif case.kind == "beam":
        plain = dec.predict_beam(a[0], case.max_len, *a[1:], beam_size=case.rps, return_all=True)
        res = dec.predict_beam(a[0], case.max_len, *a[1:], beam_size=case.rps, return_all=True, return_attention=True)
        for x, y in zip(plain, res[:4]):
            assert torch.equal(x, y), case.name
        best, hyp = res[4].cpu(), res[5].cpu()
        assert hyp.shape == (case.max_len, case.B, case.rps, case.layers, case.H, case.S)
        bi = res[3].argmax(dim=1).cpu()
        assert torch.equal(best, hyp[:, torch.arange(case.B), bi]), case.name
        seqs = res[2].cpu().reshape(case.R, case.max_len)
        fed, live = prefix_feeds(seqs, cfg.start, cfg.end)
        ref = cross_weights(fp64, fed, torch.arange(case.R) // case.rps)
        worst = check_weights(case.name, hyp.reshape(case.max_len, case.R, *hyp.shape[3:]), ref, live)
    else:
        kw = dict(num_samples=case.rps, temperature=1.0, top_k=8, top_p=0.9, seed=11, return_log_probs=True)
        s0, l0 = dec.predict_sample(a[0], case.max_len, *a[1:], **kw)
        s1, l1, attn = dec.predict_sample(a[0], case.max_len, *a[1:], return_attention=True, **kw)
        assert torch.equal(s0, s1) and torch.equal(l0, l1), case.name
        fed, live = prefix_feeds(s1.t().cpu(), cfg.start, cfg.end)
        ref = cross_weights(fp64, fed, torch.arange(case.R) // case.rps)
        worst = check_weights(case.name, attn.cpu(), ref, live)
    print("%s: max |weight - fp64| %.2e" % (case.name, worst))


@pytest.mark.parametrize("name", [c.name for c in CASES])
def test_attention_envelope(name):
    run_case(BY_NAME[name])


def test_attention_greedy_gemm_split(gemm_split):
    run_case(BY_NAME["greedy_b32"])


# ------------------------------------------------------------------------------------------------ nothing else changes
def test_replay_and_alternation_are_bit_identical():
    case = Case("alt", "greedy", 5, max_len=10)
    dec, cfg, P, ents, facts, enc = build(case)
    a = args_of(enc, ents, facts)
    g0 = dec.predict(a[0], case.max_len, *a[1:])
    g1, w1 = dec.predict(a[0], case.max_len, *a[1:], return_attention=True)
    g2, w2 = dec.predict(a[0], case.max_len, *a[1:], return_attention=True)          # replay
    g3 = dec.predict(a[0], case.max_len, *a[1:])
    g4, w4 = dec.predict(a[0], case.max_len, *a[1:], return_attention=True)
    assert w1.data_ptr() != w2.data_ptr()                                             # callers own their copy
    for g in (g1, g2, g3, g4):
        assert torch.equal(g, g0)
    assert torch.equal(w1, w2) and torch.equal(w1, w4)
    b0 = dec.predict_beam(a[0], case.max_len, *a[1:], beam_size=3, return_all=True)
    b1 = dec.predict_beam(a[0], case.max_len, *a[1:], beam_size=3, return_all=True, return_attention=True)
    b2 = dec.predict_beam(a[0], case.max_len, *a[1:], beam_size=3, return_all=True)
    b3 = dec.predict_beam(a[0], case.max_len, *a[1:], beam_size=3, return_all=True, return_attention=True)
    for x, y, z, u in zip(b0, b1, b2, b3):
        assert torch.equal(x, y) and torch.equal(x, z) and torch.equal(x, u)
    assert torch.equal(b1[4], b3[4]) and torch.equal(b1[5], b3[5])
    kw = dict(num_samples=2, seed=5, return_log_probs=True)
    s0 = dec.predict_sample(a[0], case.max_len, *a[1:], **kw)
    s1 = dec.predict_sample(a[0], case.max_len, *a[1:], return_attention=True, **kw)
    s2 = dec.predict_sample(a[0], case.max_len, *a[1:], **kw)
    s3 = dec.predict_sample(a[0], case.max_len, *a[1:], return_attention=True, **kw)
    for x, y, z, u in zip(s0, s1, s2, s3):
        assert torch.equal(x, y) and torch.equal(x, z) and torch.equal(x, u)
    assert torch.equal(s1[2], s3[2])


# ------------------------------------------------------------------------------------------------ beam ancestry
def test_beam_weights_follow_the_ancestry(monkeypatch):
    """Hypotheses change parents: every final hypothesis's gathered weights match fp64 on its own prefix, and reading
    the final row's own buffer instead (no gather through the ancestry table) does not."""
    case = Case("anc", "beam", 4, rps=4, max_len=12, end_bias=-30.0)
    dec, cfg, P, ents, facts, enc = build(case)
    dec.use_hip_graphs = False
    bufs = []
    real = ops.decode_layers_attn

    def spy(ctx, attn, pos, part=0):
        if attn is not None and (not bufs or bufs[-1] is not attn):
            bufs.append(attn)
        return real(ctx, attn, pos, part)

    monkeypatch.setattr(ops, "decode_layers_attn", spy)
    a = args_of(enc, ents, facts)
    res = dec.predict_beam(a[0], case.max_len, *a[1:], beam_size=case.rps, return_all=True, return_attention=True)
    assert len(bufs) == 1
    raw, hyp = bufs[0].cpu(), res[5].cpu().reshape(case.max_len, case.R, case.layers, case.H, case.S)
    seqs = res[2].cpu().reshape(case.R, case.max_len)
    fed, live = prefix_feeds(seqs, cfg.start, cfg.end)
    assert min(live) == case.max_len                        # no hypothesis ends: all 12 steps compared
    ref = cross_weights(Fp64Decode(cfg, P, enc, ents, facts), fed, torch.arange(case.R) // case.rps)
    check_weights("anc", hyp, ref, live)
    no_gather = np.abs(raw.double().numpy().transpose(1, 0, 2, 3, 4) - ref).max()
    assert no_gather > 100 * ATOL, ("the case does not reorder hypotheses", no_gather)


# ------------------------------------------------------------------------------------------------ early exit
def test_every_row_ends_early():
    case = Case("early", "greedy", 3, max_len=12, end_bias=8.0)
    dec, cfg, P, ents, facts, enc = build(case)
    a = args_of(enc, ents, facts)
    seq, attn = dec.predict(a[0], case.max_len, *a[1:], return_attention=True)
    live = live_steps(seq.t().cpu(), cfg.end)
    last = max(live)
    assert last < case.max_len, live
    assert (attn[last:] == 0).all()
    out, fed, raw = greedy_production_attn(dec, enc, ents, facts, case.max_len)
    assert (raw[last + 1:] == 0).all()                      # the kernels skipped those steps: nothing was written
    ref = cross_weights(Fp64Decode(cfg, P, enc, ents, facts), fed, torch.arange(case.B))
    check_weights("early", attn.cpu(), ref, live)


# ------------------------------------------------------------------------------------------------ memory split
@pytest.mark.parametrize("name", ["greedy_knowledge_b67", "greedy_s1024_geo"])
def test_split_lines_up_with_fp64_argmax(name):
    case = BY_NAME[name]
    dec, cfg, P, ents, facts, enc = build(case)
    a = args_of(enc, ents, facts)
    seq, attn = dec.predict(a[0], case.max_len, *a[1:], return_attention=True)
    out, fed, _ = greedy_production_attn(dec, enc, ents, facts, case.max_len)
    ref = cross_weights(Fp64Decode(cfg, P, enc, ents, facts), fed, torch.arange(case.B))
    parts = D.split_attention(attn.cpu(), 196, case.K, case.F)
    assert parts["image"].shape[-2:] == (14, 14) and parts["entities"].shape[-1] == case.K
    assert parts["facts"].shape[-1] == case.F
    live = live_steps(out, cfg.end)
    hits = {"image": 0, "entities": 0, "facts": 0}
    for r, n in enumerate(live):
        am = ref[r, :n].argmax(-1)                                   # (n, layers, H)
        for (i, l, h), s in np.ndenumerate(am):
            if s < 196:
                v, key = parts["image"][i, r, l, h, s // 14, s % 14], "image"
            elif s < 196 + case.K:
                v, key = parts["entities"][i, r, l, h, s - 196], "entities"
            else:
                v, key = parts["facts"][i, r, l, h, s - 196 - case.K], "facts"
            assert abs(float(v) - ref[r, i, l, h, s]) < ATOL, (name, r, i, l, h, s)
            hits[key] += 1
    print(name, "fp64 argmax rows by segment", hits)
    assert sum(hits.values()) > 0


# ------------------------------------------------------------------------------------------------ evaluate
@pytest.mark.parametrize("sample", [None, dict(num_samples=2, seed=3)], ids=["greedy", "sample"])
def test_evaluate_writes_attention(tmp_path, sample):
    from ick_amd import eval as ev
    from ick_amd import synth
    from ick_amd.datasets import CaptionDataset
    from test_bench_sizes_gpu import make_encoder
    from test_sample_gpu import build_decoder
    V, variant = 60, "knowledge"
    data_dir = str(tmp_path / "data")
    wm = synth.write_dataset(data_dir, "toy", variant, n_train=4, n_val=2, n_test=5, L=12, K=6, V=V, F=5)
    dec = build_decoder(variant, V, synth.make_params(variant, V, 2))
    enc, _, _ = make_encoder(2)
    loader = torch.utils.data.DataLoader(CaptionDataset(data_dir, "toy", "TEST"), batch_size=5, shuffle=False)
    path = str(tmp_path / "attn.npz")
    caps, seqs = ev.evaluate(enc, dec, loader, wm, max_caption_len=10, out_csv=str(tmp_path / "c.csv"), sample=sample,
                             attention_out=path)
    caps0, seqs0 = ev.evaluate(enc, dec, loader, wm, max_caption_len=10, out_csv=None, sample=sample)
    assert seqs == seqs0
    z = np.load(path)
    n = 5 * (1 if sample is None else 2)
    assert z["attention"].shape == (n, 10, 196 + 6 + 5) and z["attention"].dtype == np.float16
    assert (int(z["P"]), int(z["K"]), int(z["F"])) == (196, 6, 5)
    assert z["tokens"].tolist() == seqs
    batch = next(iter(loader))
    image = batch[0].cuda()
    enc_in = image if image.dim() == 4 and image.shape[1] == enc.encoder_dim else enc(image)
    if sample is None:
        _, attn = dec.predict(enc_in, 10, batch[4], batch[6].cuda(), return_attention=True)
    else:
        _, attn = dec.predict_sample(enc_in, 10, batch[4], batch[6].cuda(), return_attention=True, **sample)
    want = attn[:, :, -1].mean(dim=2).transpose(0, 1).to(torch.float16).cpu().numpy()
    assert np.array_equal(z["attention"], want)


# ------------------------------------------------------------------------------------------------ errors
def test_unsupported_sizes_raise_before_capture():
    case = Case("outside", "greedy", 2, K=829, max_len=8, V=300)            # S = 1025
    dec, cfg, P, ents, facts, enc = build(case)
    e = enc.cuda()
    with pytest.raises(IckError):
        dec.predict(e, 8, ents, return_attention=True)
    with pytest.raises(IckError):
        dec.predict_beam(e, 8, ents, beam_size=3, return_attention=True)
    with pytest.raises(IckError):
        dec.predict_sample(e, 8, ents, num_samples=2, seed=1, return_attention=True)
    ok = Case("ok", "greedy", 2, max_len=8, V=300)
    dec, cfg, P, ents, facts, enc = build(ok)
    e = enc.cuda()
    dec.fused_decode = False
    with pytest.raises(IckError):
        dec.predict(e, 8, ents, return_attention=True)
    dec.fused_decode = True
    limit = D.ATTENTION_MAX_BYTES
    try:
        D.ATTENTION_MAX_BYTES = 1024
        with pytest.raises(IckError):
            dec.predict(e, 8, ents, return_attention=True)
        with pytest.raises(IckError):
            dec.predict_beam(e, 8, ents, beam_size=3, return_attention=True)
        with pytest.raises(IckError):
            dec.predict_sample(e, 8, ents, num_samples=2, seed=1, return_attention=True)
    finally:
        D.ATTENTION_MAX_BYTES = limit
    assert not dec.__dict__.get("_graphs")                                   # nothing was captured
