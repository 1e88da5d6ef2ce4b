"""The training step with dropout ON against the float64 masked oracle (oracle/restatement.py, drop=).

ick_dropout_mask reports what a kernel drops for a (p, seed, site); the kernels key their masks by the logical element
index and add the device step counter to the seed (epoch_seed(), csrc/common.h).  So the oracle can play the step's own
masks back, and the whole composition -- which site a launch regenerates, with which rate and keep-scale, under which
counter value, indexed how -- is compared with something other than itself.

Level A: forward_with_tape / backward_from_tape called directly (literal seed, a counter tensor holding 3), every
parameter gradient by name.  Level B: the captured TrainStep over three steps on two alternating batches, lr = 0 so the
weights stay put while the counter advances.

Bars, from the dropout-off comparisons with the same oracle (tests/test_bench_sizes_gpu.py): loss 2e-5; gradients 2e-3 of
max(1e-3, |ref|max) per tensor with the ReLU-flip allowance of run_train_step_vs_oracle; scores 2e-4 * max(1, |ref|max).
The float32 evaluation of the masked oracle on the CPU stays within 2.3e-6 (relative, gradients) and 3.2e-6 (scores) of
its float64 evaluation at every point used here and sets no hidden unit aside (tests/test_dropout_oracle_cpu.py checks
that); on the MI355X the kernels came within 2.6e-6 and 3.6e-6, losses within 5e-7, no unit set aside.
"""
import pytest
import torch

import dropout_ref as DR
from test_forward_gpu import build_decoder
from test_training_gpu import reference_loss

pytestmark = pytest.mark.gpu


@pytest.fixture()
def ops():
    import ick_amd.ops as o
    return o


def build(case, chains=True):
    dec = DR.set_rates(build_decoder(case["variant"], DR.V, case["P"]).train(), case["rates"])
    assert dec.chain_supported() and dec.chain_bwd_supported()
    if not chains:
        dec.__dict__["_chain_ok"] = False
        dec.__dict__["_chain_bwd_ok"] = False
    return dec


def tape_inputs(dec, case):
    """-> (captions, masks, entities, facts, enc_tok) on the device, as forward_with_tape takes them."""
    b = case["batch"]
    facts = b["facts"].cuda() if "facts" in b else None
    enc, ents, facts = dec._prepare_inputs(case["enc_out"].cuda(), b["entities"], facts)
    return b["captions"].cuda(), b["caption_masks"].cuda(), ents, facts, dec._token_major(enc).contiguous()


def module_args(case):
    b = case["batch"]
    x = case["feats"].cuda() if "feats" in case else case["enc_out"].cuda()
    args = [b["captions"].cuda(), x, b["caption_masks"].cuda(), b["caption_lengths"].cuda(), b["entities"]]
    if "facts" in b:
        args.append(b["facts"].cuda())
    return args


_REFS = {}


def reference(case, table, epoch_value, ops):
    """The masked oracle's step for (case, sites, counter value): the same for every product mode of the GEMM tiles and
    for the chained and the unfused path, so it is shared between them; the last few are kept."""
    key = (case["name"], tuple(DR.triples(table)), epoch_value)
    if key not in _REFS:
        if len(_REFS) >= 6:
            _REFS.clear()
        masks = DR.masks_from_table(table, epoch_value, ops.dropout_mask)
        assert all(0.0 < (m > 0).double().mean().item() < 1.0 for m in masks.values())
        _REFS[key] = DR.masked_reference(case, masks)
    return _REFS[key]


def check_table(table, case, seed, epoch):
    """What the tape says about the sites of one step: distinct ids, one seed, the counter tensor on every tuple, and
    each site's own module rate."""
    DR.assert_sites_distinct(table)
    for e in table:
        p = case["rates"][e["name"]]
        assert e["drop"] is not None and e["drop"][0] == float(p), (e["name"], e["drop"], p)
        assert e["drop"][1] == seed, (e["name"], e["drop"], seed)
        if epoch is None:
            assert len(e["drop"]) == 3, e["name"]
        else:
            assert len(e["drop"]) == 4 and e["drop"][3] is epoch, e["name"]


# ------------------------------------------------------------------------------------------------ the mask restatement
@pytest.mark.parametrize("rows,cols,p,seed,site", [(45, 300, 0.5, 0x5EED1234, 1), (450, 202, 0.1, 0xFFFFFFFF, 31),
                                                   (45, 512, 0.325, 7, 0x01000000), (300, 9, 0.6, 0, 17)])
def test_hash_mask_is_the_kernels_mask(ops, rows, cols, p, seed, site):
    """The numpy restatement the CPU tests draw masks with == ick_dropout_mask, bit for bit (seed + counter wraps)."""
    for ep in (0, 3):
        got = ops.dropout_mask(rows, cols, p, (seed + ep) & 0xFFFFFFFF, site).cpu()
        assert torch.equal(got, DR.hash_mask(rows, cols, p, (seed + ep) & 0xFFFFFFFF, site))


# ------------------------------------------------------------------------------------------------ level A: the eager tape
def run_tape(ops, name, chains=True):
    from ick_amd.training import backward_from_tape, forward_with_tape, unique_parameters
    case = DR.make_case(name)
    dec = build(case, chains)
    caps, masks, ents, facts, enc_tok = tape_inputs(dec, case)
    epoch = torch.tensor([DR.TAPE_EPOCH], device="cuda", dtype=torch.int32)
    scores, tape = forward_with_tape(dec, caps, masks, ents, facts, enc_tok, None, seed=DR.TAPE_SEED, epoch=epoch)
    assert (tape.misc.get("pkb") is not None) == chains
    table = DR.table_from_tape(tape, case["variant"], case["B"], case["Fn"])
    check_table(table, case, DR.TAPE_SEED, epoch)
    ref = reference(case, table, DR.TAPE_EPOCH, ops)
    what = "tape %s%s" % (name, "" if chains else " (chains off)")
    DR.check_scores(scores, ref, what)
    dl = torch.tensor(ref["decode_lengths"], dtype=torch.int32, device="cuda")
    ls, cnt, _ = ops.packed_ce(scores, caps, dl, case["cfg"].pad, want_grad=False)
    loss = ls.item() / cnt.item()
    print("%s: loss %.7f, oracle %.7f" % (what, loss, ref["loss"]))
    assert cnt.item() == sum(ref["decode_lengths"]) and abs(loss - ref["loss"]) < DR.LOSS_BAR
    # the oracle's own gradient of the token-mean loss with respect to the scores, on both sides; in the padded row
    # stride the score head writes
    B, Lc, Vx = scores.shape
    dsc = torch.zeros(B, Lc, scores.stride(1), device="cuda")[:, :, :Vx]
    dsc.copy_(ref["dscores"].float())
    grads = {id(p): torch.zeros_like(p) for p in unique_parameters(dec)}
    backward_from_tape(dec, tape, dsc, grads)
    torch.cuda.synchronize()
    DR.check_grads({k: grads[id(p)] for k, p in dec.named_parameters()}, ref["grads"], what)


@pytest.mark.parametrize("name", ["geo", "knowledge", "news", "geo_distinct_rates"])
def test_tape_vs_masked_oracle(ops, name, gemm_split):
    """Scores at every valid position, the loss and every parameter gradient of forward_with_tape + backward_from_tape
    (train mode, counter at 3).  geo_distinct_rates gives each of the 31 dropout modules its own rate in 0.05 .. 0.6: a
    launch that takes a neighbour's rate or keep-scale (all equal at the reference's rates) changes the numbers."""
    run_tape(ops, name)


def test_tape_vs_masked_oracle_chains_off(ops):
    """The unfused path (separate GEMM / add & norm / LayerNorm-backward kernels) hands out and regenerates the same
    sites."""
    run_tape(ops, "geo", chains=False)


def test_autograd_bridge_vs_masked_oracle(ops, monkeypatch):
    """dec(*args) in train() mode + loss.backward(): the seed is (_drop_seed * 2654435761 + _drop_step) mod 2^32
    (DecoderGraphFn.forward), no counter.  The second call of the module draws other masks and still matches."""
    from ick_amd import training
    case = DR.make_case("geo")
    dec = build(case)
    taped = []
    inner = training.forward_with_tape

    def spy(*a, **kw):
        out = inner(*a, **kw)
        taped.append((out[1], kw))
        return out

    monkeypatch.setattr(training, "forward_with_tape", spy)
    args = module_args(case)
    named = dict(dec.named_parameters())
    seen = []
    for call in (1, 2):
        dec.zero_grad(set_to_none=True)
        scores, caps, dl = dec(*args)
        assert len(taped) == call and dec.__dict__["_drop_step"] == call
        tape, kw = taped[-1]
        seed = (dec.__dict__.get("_drop_seed", 0x1234567) * 2654435761 + dec.__dict__["_drop_step"]) & 0xFFFFFFFF
        assert kw["seed"] == seed == DR.bridge_seed(call) and kw.get("epoch") is None
        table = DR.table_from_tape(tape, case["variant"], case["B"], case["Fn"])
        check_table(table, case, seed, None)
        ref = reference(case, table, 0, ops)
        what = "autograd bridge, call %d" % call
        assert dl == ref["decode_lengths"] and torch.equal(caps.cpu(), case["batch"]["captions"])
        DR.check_scores(scores, ref, what)
        loss = reference_loss(scores, caps, dl, case["cfg"].pad)
        assert abs(loss.item() - ref["loss"]) < DR.LOSS_BAR, (what, loss.item(), ref["loss"])
        loss.backward()
        DR.check_grads({k: (p.grad if p.grad is not None else torch.zeros_like(p)) for k, p in named.items()},
                       ref["grads"], what)
        seen.append(ref["loss"])
    assert abs(seen[0] - seen[1]) > 1e-3       # other masks: the two calls are two different functions


# ------------------------------------------------------------------------------------------------ level B: TrainStep
def run_steps(ops, monkeypatch, name_a, name_b, lazy=False):
    """Three captured steps on batches a, b, a with lr = 0: after each, the returned loss and the gradient bucket against
    the masked oracle at the counter value that step's forward saw.

    When the counter moves (training.py): the eager order runs graph A (_part_a: forward, loss, backward), then graph B
    (_part_b: Adam, then ick_counter_add) -- every kernel of step i reads i, and the step returns with i + 1.  With
    lazy_update the bump (ick_counter_add_if, after the deferred Adam) sits at the head of the NEXT step's graph A, on the
    side stream before anything reads a parameter: the step returns with the counter it ran under, the first one (no
    update pending: the token count is zero) runs under 0 -- so step i's kernels, forward and backward, read i as well."""
    from ick_amd import decoder as decmod
    from ick_amd.training import TrainStep, forward_with_tape
    cases = [DR.make_case(name_a), DR.make_case(name_b)]
    a = cases[0]
    assert all(torch.equal(cases[1]["P"][k], v) for k, v in a["P"].items())
    dec = build(a)
    enc = None
    if "feats" in a:
        from test_bench_sizes_gpu import make_encoder
        enc, cw, cb = make_encoder(a["pseed"])
        assert torch.equal(cw, a["conv1"][0]) and torch.equal(cb, a["conv1"][1])
    log = []
    inner = decmod.DropSites.site

    def spy(self, p):
        out = inner(self, p)
        log.append(out)
        return out

    monkeypatch.setattr(decmod.DropSites, "site", spy)
    # the sites by name, from an eager tape on the same inputs, seed and a stand-in counter
    seed = DR.step_seed()
    stand_in = torch.zeros(1, device="cuda", dtype=torch.int32)
    tables = []
    for c in cases:
        eager = dict(c)
        if "feats" in c:
            with torch.no_grad():
                eager["enc_out"] = enc(c["feats"].cuda())
        with torch.no_grad():
            _, tape = forward_with_tape(dec, *tape_inputs(dec, eager), None, seed=seed, epoch=stand_in)
        tables.append(DR.table_from_tape(tape, c["variant"], c["B"], c["Fn"]))
        check_table(tables[-1], c, seed, stand_in)
    n_sites = len(tables[0])
    assert len(log) == 2 * n_sites and DR.triples(tables[0]) == DR.triples(tables[1])
    del log[:]
    ts = TrainStep(dec, lr=0.0, grad_clip=5.0, seed=DR.STEP_SEED, encoder=enc, lazy_update=lazy)
    named = dict(dec.named_parameters())
    p0 = ts.flat_p.clone()
    for i in range(3):
        c, table = cases[i % 2], tables[i % 2]
        before = int(ts.counter.item())
        loss = ts(*module_args(c)).item()
        torch.cuda.synchronize()
        after = int(ts.counter.item())
        if lazy:
            assert ts._pending and (before, after) == (max(i - 1, 0), i), (i, before, after)
        else:
            assert (before, after) == (i, i + 1), (i, before, after)
        saw = i
        if i == 0:
            # the warm-up pass and the captured pass each handed out the eager tape's sites, with the step's counter
            assert ts.use_graph, "hipGraph capture failed: the captured step was not exercised"
            assert len(log) == 2 * n_sites, len(log)
            for half in (log[:n_sites], log[n_sites:]):
                assert [t[:3] for t in half] == [e["drop"][:3] for e in sorted(tables[0], key=lambda e: e["drop"][2])]
                assert all(len(t) == 4 and t[3] is ts.counter for t in half)
        else:
            assert len(log) == 2 * n_sites, "a later step captured again instead of replaying"
        ref = reference(c, table, saw, ops)
        what = "TrainStep %s step %d (counter %d)%s" % (c["name"], i + 1, saw, ", lazy update" if lazy else "")
        print("%s: loss %.7f, oracle %.7f" % (what, loss, ref["loss"]))
        assert abs(loss - ref["loss"]) < DR.LOSS_BAR, (what, loss, ref["loss"])
        if lazy:
            # the update is still pending: the bucket holds the sum over tokens, not yet divided and clamped
            count = ts.flat_g[ts._t + 1].item()
            assert count == sum(ref["decode_lengths"])
            mine = {k: (ts.grads[id(p)] / count).clamp(-5.0, 5.0) for k, p in named.items()}
        else:
            # after the step the bucket holds what Adam consumed: the token-mean gradient, clamped to +-5
            mine = {k: ts.grads[id(p)] for k, p in named.items()}
        DR.check_grads(mine, ref["grads"], what, clamp=5.0)
    assert torch.equal(ts.flat_p, p0)          # lr = 0: every step ran on the same weights
    return ts


@pytest.mark.parametrize("name", ["geo", "knowledge"])
def test_train_step_vs_masked_oracle(ops, monkeypatch, name, gemm_split):
    run_steps(ops, monkeypatch, name, name + "_b")


def test_train_step_bench_composition_vs_masked_oracle(ops, monkeypatch):
    """What the benchmark runs: TrainStep(encoder=..., lazy_update=True) fed the (B, 2048, 14, 14) feature map, B = 4.
    Steps 2 and 3 run behind the deferred update and its counter bump at the head of their own graph."""
    ts = run_steps(ops, monkeypatch, "bench", "bench_b", lazy=True)
    assert ts.derived is not None


def test_train_step_with_a_caption_of_length_one(ops, monkeypatch):
    """One caption of length 1 in the batch: a sample without a valid row (decode length 0) still draws its masks and
    contributes nothing."""
    run_steps(ops, monkeypatch, "geo_length1", "geo_length1_b")
