"""weights.WeightImages: the one owner of the decoder's re-laid-out weight copies.
  * every group notices an in-place write to one of its parameters and is re-filled IN PLACE (captured graphs and the
    optimizer kernel's table hold the addresses), bit-identical to an independent re-layout of the live parameters;
  * refresh(subset=) writes exactly the chain images it names;
  * a TrainStep whose decoder lost its owner object rebuilds its tables and graphs instead of writing freed buffers;
  * a checkpoint carries none of the caches and leaves the live decoder's alone.
"""
import pytest
import torch

import ick_amd.ops as ops
import ick_amd.synth as synth
import ick_amd.utils as utils
from ick_amd.decoder import _CACHE_KEYS
from ick_amd.training import TrainStep
from ick_amd.weights import WeightImages, first_stage
from test_forward_gpu import build_decoder
from test_training_gpu import zero_dropout

pytestmark = pytest.mark.gpu


def _decoder(variant, V=200, seed=3):
    return build_decoder(variant, V, synth.make_params(variant, V, seed))


def _buffers(wi):
    """name -> every buffer the owner holds (the flat buffers behind the packed views, not the views)."""
    out = {("flat", g): b for g, b in wi.flat.items()}
    for g, img in wi.img.items():
        out.update({(g, k): b for k, b in img.items() if g not in wi.flat})
    return out


def _reference(dec, wi, before):
    """The images an independent re-layout of the live parameters gives: torch for the plain copies, the stand-alone
    kernels into fresh buffers (copies of the images before the write: any byte a kernel leaves alone is equal) else."""
    d = dec.emb_dim
    layers = dec.transformer_decoder.layers
    ref = {("kv", "wkv"): torch.cat([l.multihead_attn.in_proj_weight.detach()[d:] for l in layers]),
           ("kv", "bkv"): torch.cat([l.multihead_attn.in_proj_bias.detach()[d:] for l in layers])}
    if dec.has_facts:
        ref[("pred_wt", "pred_wt")] = dec.fc_predicate.weight.detach().t().contiguous()
    for li, l in enumerate(layers):
        for name, mod in (("so", l.self_attn.out_proj), ("co", l.multihead_attn.out_proj), ("l2", l.linear2)):
            ref[("decode", (li, name))] = mod.weight.detach().t().contiguous()
    # the packed images, from a list of the chains' weights written out here (not the table under test), in buffer order:
    # decoder layers [so, cq, co, l1, l2, si from layer 1 on], then the context stacks [so, l1, l2, si from layer 1 on]
    views = []
    stacks = [("d", dec.transformer_decoder), ("e", dec.transformer_encoder_entities)]
    if dec.has_facts:
        stacks.append(("f", dec.transformer_encoder_facts))
    for tag, stack in stacks:
        for li, l in enumerate(stack.layers):
            views.append(((tag, li, "so"), l.self_attn.out_proj.weight.detach()))
            if tag == "d":
                views.append(((tag, li, "cq"), l.multihead_attn.in_proj_weight.detach()[:d]))
                views.append(((tag, li, "co"), l.multihead_attn.out_proj.weight.detach()))
            views += [((tag, li, "l1"), l.linear1.weight.detach()), ((tag, li, "l2"), l.linear2.weight.detach())]
            if li > 0:
                views.append(((tag, li, "si"), l.self_attn.in_proj_weight.detach()))
    for g, vs in (("chain", views),
                  ("chain_t", [(k[:2] + (k[2] + "T",), v.t()) for k, v in views] + [(("kv", "T"), ref[("kv", "wkv")].t())])):
        flat = ref[("flat", g)] = before[("flat", g)].clone()
        off = 0
        assert [k for k, _ in vs] == list(getattr(wi, g))
        for k, src in vs:
            n = ops.packed_weight_floats(*src.shape)
            ops.pack_weights([(src, flat[off:off + n])])
            assert getattr(wi, g)[k].data_ptr() == wi.flat[g].data_ptr() + 4 * off and getattr(wi, g)[k].numel() == n, k
            off += n
        assert off == flat.numel()
    w = dec.fc_vocab.weight.detach()
    for name, src in ((("kv_ps", "wkv"), ref[("kv", "wkv")]), (("vocab_ps", "vocab"), w), (("vocab_t_ps", "vocab_t"), w.t())):
        ref[name] = before[name].clone()
        ops.presplit_weights([(src, ref[name])])
    return ref


@pytest.mark.parametrize("variant", ["geo", "knowledge"])
def test_every_group_notices_a_write_and_refreshes_in_place(variant, monkeypatch):
    dec = _decoder(variant)
    wi = dec.weight_images().current(*WeightImages.GROUPS)
    assert dec.weight_images() is wi and set(wi.stamp) == set(WeightImages.GROUPS)
    torch.cuda.synchronize()
    before = {k: b.clone() for k, b in _buffers(wi).items()}
    ptrs = {k: b.data_ptr() for k, b in _buffers(wi).items()}
    l1 = dec.transformer_decoder.layers[1]
    with torch.no_grad():       # one source parameter of every group (kv / kv_ps / chain_t; chain; decode; the planes; pred_wt)
        l1.multihead_attn.in_proj_weight.mul_(1.5)
        l1.multihead_attn.in_proj_bias.add_(0.25)
        dec.transformer_encoder_entities.layers[2].linear1.weight.mul_(0.5)
        l1.linear2.weight.mul_(1.25)
        dec.fc_vocab.weight.mul_(0.75)
        if dec.has_facts:
            dec.fc_predicate.weight.mul_(2.0)
    assert all(wi.stamp[g] != wi.key(g) for g in WeightImages.GROUPS if wi.groups[g])
    ref = _reference(dec, wi, before)
    calls = []
    for name in ("pack_weights", "presplit_weights"):
        monkeypatch.setattr(ops, name, lambda *a, _f=getattr(ops, name), _n=name, **kw: (calls.append(_n), _f(*a, **kw))[1])
    assert dec.weight_images().current(*WeightImages.GROUPS) is wi
    # one launch per kind, and one more packing launch for ("kv", "T"), which is made from the kv weight gathered by the first
    assert calls == ["pack_weights", "pack_weights", "presplit_weights"]
    torch.cuda.synchronize()
    now = _buffers(wi)
    assert set(now) == set(ref) == set(before)
    for k, b in now.items():
        assert b.data_ptr() == ptrs[k], k
        assert torch.equal(b, ref[k]), (variant, k)
    changed = {k[1] if k[0] == "flat" else k[0] for k, b in now.items() if not torch.equal(b, before[k])}
    assert changed == {g for g in WeightImages.GROUPS if wi.groups[g]}      # ... and the writes did reach every group
    stamp = dict(wi.stamp)
    wi.current(*WeightImages.GROUPS)
    assert len(calls) == 3 and wi.stamp == stamp                      # nothing changed: no launch


def test_vocabulary_planes_are_handed_out_from_256_rows_on():
    dec = _decoder("geo")
    assert dec._vocab_presplit(255) is None and "vocab_ps" not in dec.weight_images().img      # B * L < 256: never asked for
    ps = dec._vocab_presplit(256)
    if ops.gemm_split_mode() == 0:
        assert ps is None
    else:
        assert ps is dec.weight_images().vocab_ps
        ref = torch.zeros_like(ps)
        mine = ps.clone()
        ops.presplit_weights([(dec.fc_vocab.weight.detach(), ref)])
        ps.zero_()
        dec.weight_images().refresh("vocab_ps")
        assert torch.equal(ps, ref) and torch.equal(mine, ref)


def test_refresh_of_a_subset_touches_only_its_images():
    dec = _decoder("knowledge")
    wi = dec.weight_images().current("chain")
    torch.cuda.synchronize()
    full = wi.flat["chain"].clone()
    wi.flat["chain"].fill_(float("nan"))
    wi.refresh("chain", subset=first_stage)
    torch.cuda.synchronize()
    first = {e.key for e in wi.groups["chain"] if first_stage(e.key)}
    assert first and len(first) < len(wi.chain)
    off = 0
    for e in wi.groups["chain"]:
        got, want = wi.chain[e.key], full[off:off + e.dst.numel()]
        off += e.dst.numel()
        if e.key in first:
            assert torch.equal(got, want), e.key
        else:
            assert torch.isnan(got).all(), e.key
    assert wi.stamp["chain"] == wi.key("chain")          # (the stamp of the full refresh: a partial one leaves it alone)
    wi.refresh("chain", subset=lambda k: not first_stage(k))
    assert torch.equal(wi.flat["chain"], full)


def test_a_replaced_owner_is_noticed_by_the_train_step():
    variant, B, L, K, V, seed = "geo", 4, 7, 6, 120, 9
    P = synth.make_params(variant, V, seed)
    b = synth.make_batch(variant, B, L, K, V, 0, seed)
    args = [b["captions"].cuda(), synth.make_enc_out(B, seed).cuda(), b["caption_masks"].cuda(),
            b["caption_lengths"].cuda(), b["entities"]]
    dec = zero_dropout(build_decoder(variant, V, P).train())
    ts = TrainStep(dec, lr=0.0)
    l_a = ts(*args).item()
    assert ts.derived is not None and ts.derived.owner is dec.weight_images() and len(ts._graphs) == 1
    old, items = ts.derived.owner, ts.derived.items_dev
    del dec.__dict__["_images"]
    l_b = ts(*args).item()
    l_ref = TrainStep(zero_dropout(build_decoder(variant, V, P).train()), lr=0.0)(*args).item()
    print("losses: before %.7f, after the owner was dropped %.7f, fresh step %.7f" % (l_a, l_b, l_ref))
    assert abs(l_b - l_ref) < 1e-5
    new = dec.weight_images()
    assert new is not old and ts.derived.owner is new and ts.derived.items_dev is not items and not ts.derived.stale
    assert len(ts._graphs) == 1          # captured again, over the new owner's buffers


def test_checkpoint_leaves_the_caches_with_the_live_decoder(tmp_path):
    variant, V, B, K = "geo", 60, 2, 6
    dec = _decoder(variant, V)
    b = synth.make_batch(variant, B, 7, K, V, 0, 5)
    dec.predict(synth.make_enc_out(B, 5).cuda(), 6, b["entities"])
    owner, graphs = dec.__dict__["_images"], dec.__dict__["_graphs"]
    assert graphs and owner.img
    path = utils.save_checkpoint("unit", 1, 0, None, dec, None, None, 0.0, False, out_dir=str(tmp_path))
    loaded = utils.load_checkpoint(path, map_location="cpu")["decoder"]
    assert not set(loaded.__dict__) & set(_CACHE_KEYS) and "_images" in _CACHE_KEYS
    assert dec.__dict__["_images"] is owner and dec.__dict__["_graphs"] is graphs and len(graphs) >= 1
    assert dec.weight_images() is owner
