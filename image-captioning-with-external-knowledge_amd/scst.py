"""Self-critical sequence training (Rennie et al. 2017, "Self-critical Sequence Training for Image Captioning").

One SelfCriticalStep call draws `num_samples` captions per image on the fused decode kernels (predict_sample's device
path), optionally decodes the greedy caption as the baseline (predict(), with its n-gram clean-up), scores every caption
with the caller's reward function, and runs one fused TrainStep on the sampled captions with the advantages as
per-caption loss weights -- the policy gradient -(r - b) * sum_t log p(w_t), divided by the token count like the cross
entropy it replaces.

The sample and greedy decode graphs belong to the step (not to the decoder's own graph cache, which every optimizer
step drops): each opens with one launch that re-derives every weight copy the decode reads from the live parameters
(DecoderTransformer._refresh_decode_copies), so the graphs stay valid across updates and are captured once per shape.

Device reward: with a cider.CiderD as reward_fn, step(..., refs=) scores every caption on the device in one launch
(ick_cider_d, SCST layout) that writes the rewards and the advantages the training step takes as caption weights --
nothing is copied to the host.  A metrics.MetricReward (CIDEr-D mixed with BLEU-n / ROUGE-L) is a device reward too:
the CiderD launch, then ick_caption_metrics on its rewards, which writes the mixed rewards and their advantages.

Dropout: sampling and the greedy decode never apply it; the teacher-forced pass uses the decoder's own mode, as TrainStep
does.  In train() mode the gradient is therefore taken at the dropout-perturbed model, not at the model that drew the
samples (the standard recipe).
"""
import collections
import struct

import torch

from . import ops
from .cider import CiderD
from .decoder import _GraphedCall
from .lib import IckError
from .metrics import MetricReward

SCSTOutput = collections.namedtuple("SCSTOutput", "loss samples rewards advantages greedy greedy_rewards sample_seed")


class SelfCriticalStep:
    """step = SelfCriticalStep(train_step, reward_fn, num_samples=5, baseline="greedy" | "mean", max_len=20, ...)
    out = step(encoder_out, entities, facts=None, refs=None)

    reward_fn(tokens, image_index) -> N floats: tokens (N, max_len) CPU LongTensor (<pad> after <end>), image_index (N,)
    CPU LongTensor.  It is called once per step over the B * n samples (row b * n + j = sample j of image b) followed,
    with baseline="greedy", by the B greedy captions.

    Returns SCSTOutput: loss (device scalar, the weighted token-mean loss), samples (B * n, max_len) and rewards (B * n,),
    advantages (B * n,), greedy (B, max_len) and greedy_rewards (B,) (None with baseline="mean"), and the sampler seed
    of this step (predict_sample(..., seed=sample_seed) reproduces the samples from the same parameters).
    reward_fn may instead be a cider.CiderD or a metrics.MetricReward: each call then needs refs, the batch's reference
    captions (B, M, Lr) or (B, L) int64, and the rewards and advantages come from the device (one launch for a CiderD,
    one more for a MetricReward's mix).  SCSTOutput then holds DEVICE tensors
    (samples, rewards, advantages, greedy, greedy_rewards) and the step never synchronises with the host.
    Advantages: "greedy" a_bj = r_bj - r_greedy_b; "mean" the leave-one-out mean a_bj = r_bj - (sum_k r_bk - r_bj)/(n-1).
    encoder_out: (B, d, P) encoder output, or the (B, 2048, 14, 14) feature map with an encoder attached to the decoder or
    given to the TrainStep (Encoder.conv1 then runs once per step at B rows).
    A TrainStep built with label_smoothing= composes as the weighted formula says: each sampled row's SMOOTHED loss and
    gradient are multiplied by its caption's advantage (the count stays unweighted); nothing here changes."""

    def __init__(self, train_step, reward_fn, num_samples=5, baseline="greedy", max_len=20, temperature=1.0, top_k=0,
                 top_p=1.0, seed=0):
        if baseline not in ("greedy", "mean"):
            raise IckError('baseline must be "greedy" or "mean"')
        if not (isinstance(num_samples, int) and num_samples >= 1):
            raise IckError("num_samples must be an integer >= 1")
        if baseline == "mean" and num_samples < 2:
            raise IckError('baseline="mean" needs num_samples >= 2')
        if not (isinstance(max_len, int) and max_len >= 1):
            raise IckError("max_len must be an integer >= 1")
        if not (temperature > 0 and temperature < float("inf")) or not (isinstance(top_k, int) and top_k >= 0) or \
                not (0 < top_p <= 1):
            raise IckError("need a finite temperature > 0, an integer top_k >= 0 and 0 < top_p <= 1")
        if getattr(train_step, "train_conv1", False):
            # the sampled captions travel with image_index over token-major encoder rows, from where the step cannot
            # reach Encoder.conv1: self-critical training with a trained projection is not supported
            raise IckError("SelfCriticalStep cannot drive a TrainStep built with train_conv1=True (its samples share "
                           "token-major encoder rows through image_index)")
        if getattr(train_step, "ss", None) is not None:
            raise IckError("SelfCriticalStep cannot drive a TrainStep built with scheduled_sampling=: it trains on sampled "
                           "captions already (and weighs them with caption_weights, which such a step refuses)")
        self.ts = train_step
        self.dec = train_step.dec
        self.reward_fn = reward_fn
        self.n, self.baseline, self.max_len = num_samples, baseline, max_len
        self.temperature, self.top_k, self.top_p = float(temperature), int(top_k), float(top_p)
        self.seed = int(seed)
        self.step_count = 0
        self.captures = 0           # decode graphs captured by this step (one per kind and shape)
        self._graphs = {}
        self._index = {}
        self.marks = None           # a list: every call appends (phase, HIP event, host time) at its phase boundaries

    def _mark(self, name):
        if self.marks is not None:
            import time
            ev = torch.cuda.Event(enable_timing=True)
            ev.record()
            self.marks.append((name, ev, time.perf_counter()))

    # ---- decode graphs that outlive optimizer steps ----------------------------------------------
    def _graphed(self, kind, key, fn, inputs, rows):
        dec = self.dec
        full = (kind, key, ops.gemm_split_mode(), self.ts.flat_p.data_ptr())
        g = self._graphs.get(full)
        if g is None or g.images is not dec.__dict__.get("_images"):      # (a graph reads its owner's buffers, and holds it)
            def body(*ins):
                dec._refresh_decode_copies(rows)
                return fn(*ins)

            if len(self._graphs) >= 8:
                self._graphs.clear()
            with torch.no_grad():
                g = _GraphedCall(body, inputs)
            self._graphs[full], g.images = g, dec.weight_images()
            self.captures += 1
        with torch.no_grad():
            return g(*inputs)

    def sample_seed(self, step):
        """The sampler seed of step `step` (a pure function of the constructor's seed and the step number)."""
        x = (self.seed * 0x9E3779B97F4A7C15 + (step + 1) * 0xBF58476D1CE4E5B9) & (2 ** 64 - 1)
        x ^= x >> 31
        return x - 2 ** 64 if x >= 2 ** 63 else x

    def _image_index(self, B, dev):
        idx = self._index.get((B, dev))
        if idx is None:
            idx = self._index[(B, dev)] = torch.arange(B, device=dev, dtype=torch.int32).repeat_interleave(self.n)
        return idx

    def __call__(self, encoder_out, entities, facts=None, refs=None):
        ts, dec, n, T = self.ts, self.dec, self.n, self.max_len
        on_device = isinstance(self.reward_fn, (CiderD, MetricReward))
        if on_device and refs is None:
            raise IckError("a CiderD or MetricReward reward needs refs= (the batch's reference captions)")
        if refs is not None and not on_device:
            raise IckError("refs= belongs to a device reward (CiderD, MetricReward); a host reward_fn takes the tokens only")
        ts.flush()                  # the decode reads the parameters: apply a pending lazy update first
        encoder_out, entities, facts = dec._prepare_inputs(encoder_out, entities, facts)
        entities = entities.contiguous()
        if encoder_out.dim() == 4:
            enc = dec.__dict__.get("_enc") or ts.enc
            if enc is None:
                raise IckError("a 4-D input is a feature map: attach an encoder to the decoder or give TrainStep encoder=")
            with torch.no_grad():
                encoder_out = enc(encoder_out.float())
        enc_tok = dec._token_major(encoder_out).contiguous()
        B, P = enc_tok.shape[0], enc_tok.shape[1]
        R = B * n
        FF = dec.transformer_decoder.layers[0].linear1.out_features
        Fn = facts.shape[1] if facts is not None else 0
        Vx = dec.vocab_size + entities.shape[1] + Fn
        if R > 65535 or not ops.decode_supported(dec.emb_dim, dec.num_heads, FF, P + entities.shape[1] + Fn, T) or \
                not ops.decode_sample_supported(Vx, n):
            raise IckError("SelfCriticalStep needs B * num_samples <= 65535 and sizes the fused decode kernels support")
        dev = enc_tok.device
        shape = (tuple(enc_tok.shape), tuple(entities.shape), None if facts is None else tuple(facts.shape), T)

        self._mark("start")
        # 1. samples (seed and knobs are graph inputs)
        seed = self.sample_seed(self.step_count)
        tp = struct.unpack("<q", struct.pack("<ff", self.temperature, self.top_p))[0]
        knobs = torch.tensor([seed, tp, min(self.top_k, 2 ** 31 - 1)], dtype=torch.int64).to(dev)
        tokens, _ = self._graphed("sample", shape + (n,),
                                  lambda t, e, f, k: dec._predict_sample_device(t, e, f, k, T, n),
                                  [enc_tok, entities, facts, knobs], R)
        self._mark("sample")
        # 2. greedy baseline: predict()'s decode, n-gram clean-up included
        greedy = None
        if self.baseline == "greedy":
            greedy = self._graphed("greedy", shape, lambda t, e, f: dec._predict_device(t, e, f, T),
                                   [enc_tok, entities, facts], B)
        self._mark("greedy")
        if on_device:
            # 3-4. rewards and advantages on the device: one launch over the sample rows and the greedy rows
            rows = torch.cat([tokens, greedy]) if greedy is not None else tokens
            rewards, adv = self.reward_fn.scst(rows, refs, n, self.baseline)
            self._mark("reward")
            return self._train(tokens, entities, facts, encoder_out, adv, adv, rows[:R], rewards[:R],
                               rows[R:] if greedy is not None else None,
                               rewards[R:] if greedy is not None else None, seed)
        # 3. rewards on the host, one call
        host = torch.cat([tokens, greedy]) if greedy is not None else tokens
        host = host.cpu()
        self._mark("to_host")
        img = torch.arange(B, dtype=torch.long).repeat_interleave(n)
        if greedy is not None:
            img = torch.cat([img, torch.arange(B, dtype=torch.long)])
        rewards = torch.as_tensor(self.reward_fn(host, img), dtype=torch.float64).reshape(-1)
        if rewards.numel() != host.shape[0]:
            raise IckError("reward_fn returned %d rewards for %d captions" % (rewards.numel(), host.shape[0]))
        r = rewards[:R].view(B, n)
        g_r = rewards[R:] if greedy is not None else None
        if self.baseline == "greedy":
            adv = r - g_r.view(B, 1)
        else:
            adv = r - (r.sum(dim=1, keepdim=True) - r) / (n - 1)
        adv = adv.reshape(-1).to(torch.float32)
        self._mark("reward")
        return self._train(tokens, entities, facts, encoder_out, adv.to(dev), adv, host[:R],
                           rewards[:R].to(torch.float32),
                           host[R:] if greedy is not None else None,
                           g_r.to(torch.float32) if g_r is not None else None, seed)

    def _train(self, tokens, entities, facts, encoder_out, weights, adv, samples, rewards, greedy, greedy_rewards,
               seed):
        """Steps 4-5; weights: the advantages on the device (the caption weights), adv: as SCSTOutput reports them."""
        ts, dec, n = self.ts, self.dec, self.n
        R = tokens.shape[0]
        B = R // n
        dev = tokens.device
        # 4. samples -> teacher-forced training rows, on the device
        wm = dec.word_map
        caps, masks, lengths = ops.samples_to_captions(tokens, dec.vocab_size, entities.shape[1], dec.has_facts,
                                                       wm["<start>"], wm["<end>"], wm["<pad>"])
        self._mark("convert")
        # 5. one weighted training step; the image rows exist once per image (image_index)
        ents_r = entities.repeat_interleave(n, dim=0)
        facts_r = facts.repeat_interleave(n, dim=0) if facts is not None else None
        loss = ts(caps, encoder_out, masks, lengths.view(R, 1), ents_r, facts_r, caption_weights=weights,
                  image_index=self._image_index(B, dev))
        self._mark("train")
        self.step_count += 1
        return SCSTOutput(loss, samples, rewards, adv, greedy, greedy_rewards, seed)
