"""Training / validation loop with the reference's structure (geo-aware/train.py:57-386; the knowledge and
news variants differ only in the extra `facts` tensors) on top of the MI355X path.

    python -m ick_amd.train  (after editing CONFIG below, like the reference's module-level globals), or
    from ick_amd import train; train.main(train.Config(variant="knowledge", data_dir=..., data_name=...))

Differences from the reference, all deliberate: images are precomputed 14x14x2048 feature maps
(datasets.CaptionDataset); `fused=True` (default) replaces Adam + clip_gradient + loss.backward() by
training.TrainStep (same update, one flat bucket, one all-reduce per step under torchrun); `fused=False` keeps the
reference's exact statement sequence (CrossEntropyLoss on pack_padded_sequence, loss.backward() through the HIP
autograd bridge, utils.clip_gradient, torch Adam).  Checkpoints use the reference's layout (utils.save_checkpoint).

SCST fine-tuning (`scst=True`, fused single-process runs only; usually from an XE checkpoint via `checkpoint`): every
TRAIN batch runs one scst.SelfCriticalStep with a CIDEr-D reward on the device (cider.CiderD, df from the TRAIN split's
captions), the batch's own captions as the references (one per image in this dataset format), in place of the
cross-entropy step.  It uses the plain fused loop, not the prefetch pipeline; validation (the cross-entropy loss) and
checkpointing are unchanged.  `scst_reward` mixes BLEU-n / ROUGE-L into that reward (metrics.MetricReward).

`val_caption_metrics=True`: validate() also decodes every validation batch greedily and scores the captions against the
batch's caption rows on the device (metrics.CaptionMetrics: BLEU-1..4, ROUGE-L, pointer precision / recall, and CIDEr-D
when a CiderD exists); the totals stay on the device until the pass ends.  `val_geo_metric=<dict>` (with it): the same
captions' geo references are counted on the device (geo_metric.GeoReferenceMetric) and their Jensen-Shannon distances
join the dict as "geo_js".

`ema_decay=<float in [0, 1)>`: an exponential moving average of the trained parameters (fused: kept by the optimizer
launch, TrainStep(ema_decay=); unfused: TorchEma, a lerp_ after optimizer.step()); with `ema_validate` the validation pass
-- and so early stopping and BEST_ -- runs on the averaged weights, and the checkpoint carries the average under
"decoder_ema" (utils.load_ema_weights copies it into a loaded checkpoint's modules).
`weight_decay=<float >= 0>`: weight decay on the decoder's matrices and embedding tables (ndim >= 2), torch.optim.AdamW's
(`decoupled_weight_decay=True`) or torch.optim.Adam(weight_decay=)'s -- fused: inside the optimizer launch
(TrainStep(weight_decay=)); unfused: the torch optimizer itself; on both the checkpoint's `decoder_optimizer` then has one
param group per parameter, and a resume takes the moments from either layout and the decay from the Config.
`scheduled_sampling_start=<epoch >= 0>`: scheduled sampling in the cross-entropy phase (fused only,
TrainStep(scheduled_sampling=)): from that epoch on each fed token is replaced with the model's own prediction with the
probability training.sampling_prob_at gives the epoch (the staircase scheduled_sampling_increase_every /
_increase_prob / _max_prob), set once per epoch through set_sampling_prob.  Validation is unchanged."""
import contextlib
import json
import math
import os
import time
from dataclasses import dataclass

import numpy as np
import torch
from torch import nn
from torch.nn.utils.rnn import pack_padded_sequence

from . import dp, load_models, ops
from . import utils as ut
from .cider import CiderD
from .datasets import CaptionDataset
from .geo_metric import GeoReferenceMetric
from .metrics import CaptionMetrics
from .scst import SelfCriticalStep
from .training import (TrainStep, check_ema_decay, check_lr_schedule, check_max_grad_norm, check_scheduled_sampling,
                       check_weight_decay, default_decay_filter, ema_decay_at, lr_at, sampling_prob_at)


@dataclass
class Config:
    variant: str = "geo"
    data_dir: str = "img_caption_data/input_dataset_files/"
    data_name: str = "geo_aware_georic2"
    pretrained_word_embeddings_file: str = ""          # GloVe text file; empty = keep the random init
    emb_dim: int = 300
    decoder_dim: int = 512
    encoder_dim: int = 512
    num_heads: int = 10
    num_layers: int = 3
    start_epoch: int = 0
    epochs: int = 120
    max_epochs_since_improvement: int = 20
    batch_size: int = 4                                # reference: 4 / 4 / 3 (geo / knowledge / news)
    workers: int = 1
    decoder_lr: float = 4e-4
    encoder_lr: float = 1e-4                           # geo-aware/train.py:47
    fine_tune_encoder: bool = False                    # geo-aware/train.py:52; True trains conv1 (+ trunk blocks 2-4)
    train_conv1: bool = False                          # train Encoder.conv1 INSIDE the fused step from a feature-file
                                                       # dataset (TrainStep(train_conv1=True, encoder_lr=encoder_lr)): what
                                                       # fine_tune_encoder=True does to a feature-file run, at the fused
                                                       # step's speed and with data parallelism; not with fine_tune_encoder,
                                                       # scst or raw images
    grad_clip: float = 5.0
    label_smoothing: float = 0.0                       # eps of the TRAINING loss, 0 <= eps < 1 (Szegedy et al. 2016; 0.1
                                                       # is usual): fused, TrainStep(label_smoothing=); unfused, torch's
                                                       # CrossEntropyLoss(label_smoothing=).  Validation stays the plain
                                                       # negative log-likelihood on both paths (val_token_metrics too), so
                                                       # early stopping and perplexity compare across values of eps
    max_grad_norm: object = None                       # float > 0: global-norm clip of the decoder's gradient before the
                                                       # element clamp grad_clip (fused, TrainStep(max_grad_norm=);
                                                       # unfused, torch.nn.utils.clip_grad_norm_); None: off
    lr_schedule: object = None                         # dict(kind="constant" | "inverse_sqrt" | "cosine" | "linear",
                                                       # warmup_steps=, total_steps=, min_lr_ratio=) on the optimizer step
                                                       # (training.lr_at); the plateau x0.8 multiplies its base rate
    print_freq: int = 100
    checkpoint: str = ""
    zero_out_epochs_since_improvement: bool = False
    fused: bool = True
    out_dir: str = "."
    max_batches: int = 0                               # >0: stop an epoch early (smoke runs)
    seed: int = 0                                      # shuffling seed shared by all ranks (torchrun)
    prefetch: bool = True                              # fused path: next batch's host-to-device copy on a copy stream
    loader_threads: int = 4                            # TRAIN batches fetched by threads of this process (0: DataLoader
                                                       # worker processes, `workers` of them, as the reference)
    half_features: bool = True                         # float16 feature files travel as float16, widened on the device
    deterministic: object = None                       # True / False: fixed-order reductions on / off; None: what
                                                       # ICK_DETERMINISTIC says at the time main() runs, else the
                                                       # library's current mode
    scst: bool = False                                 # self-critical fine-tuning with a device CIDEr-D reward
    scst_samples: int = 5                              # sampled captions per image
    scst_baseline: str = "greedy"                      # "greedy" | "mean" (leave-one-out)
    val_token_metrics: bool = False                    # validate() through decoder.score_captions: also perplexity and
                                                       # top-1 / top-5 token accuracy (STATS["val_perplexity"], ...)
    val_caption_metrics: bool = False                  # validate() also decodes every batch (predict(), max_len = the
                                                       # caption row length) and returns (loss, CaptionMetrics.result()
                                                       # dict): BLEU-1..4, ROUGE-L, pointer precision / recall on token
                                                       # ids, plus CIDEr-D under scst (STATS["caption_metrics"])
    scst_reward: object = None                         # dict of CaptionMetrics.reward()'s keyword arguments without
                                                       # `cider` (cider_weight=, bleu=, rouge_l=): the SCST reward is that
                                                       # mix around the script's CiderD; None: CIDEr-D alone
    val_geo_metric: object = None                      # dict of GeoReferenceMetric's arguments after the word map
                                                       # (bins_distance=, bins_azimuth=, n_types=, train_distribution=,
                                                       # seed=; GeoReferenceMetric.constructor_data() makes one): with
                                                       # val_caption_metrics the decoded captions' geo references are
                                                       # counted too, "geo_js" in that dict; None: off
    ema_decay: object = None                           # float in [0, 1): keep an exponential moving average of the trained
                                                       # parameters (fused: inside the optimizer launch,
                                                       # TrainStep(ema_decay=); unfused: lerp_ after optimizer.step()); the
                                                       # checkpoint then carries it under "decoder_ema"
                                                       # (utils.load_ema_weights); None: off
    ema_warmup: bool = False                           # the decay of step t is min(ema_decay, (1 + t) / (10 + t))
    ema_validate: bool = True                          # with ema_decay: validate (early stopping, BEST_) on the averaged
                                                       # weights instead of the raw ones
    weight_decay: object = None                        # float >= 0: weight decay on the decoder's parameters with
                                                       # ndim >= 2 (fused: inside the optimizer launch,
                                                       # TrainStep(weight_decay=); unfused: the torch optimizer's, over one
                                                       # param group per parameter); None: off
    decoupled_weight_decay: bool = True                # True: torch.optim.AdamW; False: torch.optim.Adam(weight_decay=)
    encoder_weight_decay: object = None                # with train_conv1: the same for Encoder.conv1.weight
    scheduled_sampling_start: int = -1                 # epoch from which fed tokens are replaced with the model's own
                                                       # predictions (fused only, TrainStep(scheduled_sampling=)); -1: off
    scheduled_sampling_increase_every: int = 5         # the probability of epoch e >= start is min(max_prob,
    scheduled_sampling_increase_prob: float = 0.05     # increase_prob * ((e - start) // increase_every + 1))
    scheduled_sampling_max_prob: float = 0.25          # (training.sampling_prob_at)
    scheduled_sampling_mode: str = "sample"            # "sample" (Gumbel-max draw at temperature 1) | "argmax"

    def __post_init__(self):
        try:
            check_ema_decay(self.ema_decay)
            check_weight_decay(self.weight_decay)
            check_weight_decay(self.encoder_weight_decay)
            check_scheduled_sampling(dict(prob=self.scheduled_sampling_max_prob, mode=self.scheduled_sampling_mode))
            check_scheduled_sampling(dict(prob=self.scheduled_sampling_increase_prob))
            sampling_prob_at(0, 0, self.scheduled_sampling_increase_every, 0.0, 0.0)
        except RuntimeError as e:
            raise ValueError(str(e))
        if self.scheduled_sampling_start >= 0 and (self.scst or not self.fused or self.fine_tune_encoder):
            raise ValueError("scheduled_sampling_start >= 0 needs the fused cross-entropy step (fused=True, "
                             "fine_tune_encoder=False, scst=False): the package has no route to the packed score rows of "
                             "the first pass outside TrainStep, and SCST trains on sampled captions already")
        if self.encoder_weight_decay is not None and not self.train_conv1:
            raise ValueError("encoder_weight_decay needs train_conv1=True")


def _batch_to_device(batch, device, has_facts):
    imgs, caps, caplens, capmasks, ent = batch[0], batch[1], batch[2], batch[3], batch[4]
    facts = batch[6].to(device) if has_facts else None
    # entity features stay on the host exactly as in geo-aware/train.py:263-266; the decoder moves them
    imgs = imgs.to(device)
    if imgs.dtype != torch.float32:                     # a float16 feature file: widened on the device
        imgs = imgs.float()
    return imgs, caps.to(device), caplens.to(device), capmasks.to(device), ent, facts


class ThreadedBatches:
    """TRAIN batches fetched and pinned by a few threads of this process, handed out in sampler order.  Worker
    PROCESSES move every 51 MB batch of float16 feature maps through shared memory (measured on the GPU box: 267 ms
    per batch with 4 workers against 37 ms fetched in-process); the copies out of the memory map and into pinned
    memory release the GIL, so threads overlap them.

    Aliasing contract.  With a FENCED consumer (one that sets `fenced = True` and leaves, for every batch it took, an event
    in `release[batch[0].data_ptr()]` after which the batch's feature tensor is no longer read -- the Prefetcher does, its
    event follows the host-to-device copy) the feature maps are written into a ring of recycled pinned blocks: a batch's
    image tensor is then only valid until that event, and is overwritten `depth + 4` batches later.  Without one
    (prefetch=False, list(loader), a batch kept for logging) every batch owns its memory, as a DataLoader's would."""

    def __init__(self, dataset, batch_sampler, threads, depth=None):
        self.dataset, self.batch_sampler, self.threads = dataset, batch_sampler, threads
        self.depth = depth or threads + 1
        # Pinned feature blocks, recycled (fenced consumers only): a batch's 26-51 MB are copied ONCE, out of the memory map
        # straight into pinned memory (round 3 copied them into a fresh numpy block and then again into a freshly allocated
        # pinned tensor).  A block is free again when the consumer's event for it has passed; the ring is deep enough that
        # this wait never triggers in steady state.  The ring pins (depth + 4) x 26-103 MB for the loader's lifetime.
        self.ring, self.ring_at = [], 0
        self.ring_size = self.depth + 4
        self.fenced = False
        self.release = {}      # data_ptr of a ring block -> event after which it may be overwritten (set by the consumer)

    def __len__(self):
        return len(self.batch_sampler)

    def _block(self, n):
        spec = getattr(self.dataset, "batch_block_spec", lambda n_: None)(n)
        if spec is None or not torch.cuda.is_available() or not self.fenced:
            return None
        shape, dt = spec
        tdt = torch.float16 if dt == np.float16 else torch.float32
        if len(self.ring) < self.ring_size:
            blk = torch.empty(shape, dtype=tdt).pin_memory()
            self.ring.append(blk)
            return blk
        blk = self.ring[self.ring_at % self.ring_size]
        self.ring_at += 1
        if tuple(blk.shape) != tuple(shape):          # the epoch's last, smaller batch: a block of its own
            return None
        ev = self.release.pop(blk.data_ptr(), None)
        if ev is not None:
            ev.synchronize()
        return blk

    def _fetch(self, idx, blk):
        batch = self.dataset.fetch_batch(idx, img_out=blk) if blk is not None else self.dataset.fetch_batch(idx)
        # the feature block is the ring's pinned memory; the small fields (a few KB each) travel pageable: pinning them
        # would be a page-locking allocation per tensor and batch
        if blk is not None:
            return batch
        return tuple(t if t.is_pinned() else t.pin_memory() for t in batch)

    def __iter__(self):
        from collections import deque
        from concurrent.futures import ThreadPoolExecutor
        pool = ThreadPoolExecutor(max_workers=self.threads)
        try:
            pending = deque()
            it = iter(self.batch_sampler)
            for idx in it:
                idx = list(idx)
                pending.append(pool.submit(self._fetch, idx, self._block(len(idx))))
                if len(pending) >= self.depth:
                    yield pending.popleft().result()
            while pending:
                yield pending.popleft().result()
        finally:
            pool.shutdown(wait=False, cancel_futures=True)


STATS = {}     # "last_epoch_steps_per_s": optimizer steps per second of the last pipelined training epoch (tools/train_rate.py)


def _batch_hook(batch):
    """Called with every host batch the Prefetcher takes from the loader (tests observe the shards through it)."""


class Prefetcher:
    """The next batch's host-to-device copies run on a copy stream while the current step computes (the loop of
    geo-aware/train.py:263-270 moves each batch synchronously in front of its step: 102.8 MB of fp32 features per 64
    samples, as long over PCIe as the whole fused step on the GPU).  Batches come out of the DataLoader pinned
    (pin_memory=True); float16 feature maps are widened on the device.  Yields the tuples _batch_to_device yields, plus
    the token count (taken from the host copy: no synchronisation)."""

    def __init__(self, loader, device, has_facts):
        # a ThreadedBatches loader recycles its pinned feature blocks for a consumer that fences their reuse (this one)
        self.release = getattr(loader, "release", None)
        if self.release is not None:
            loader.fenced = True
        self.it = iter(loader)
        self.device, self.has_facts = device, has_facts
        self.stream = torch.cuda.Stream(device)
        self.next = None
        self._load()

    def _load(self):
        try:
            batch = next(self.it)
        except StopIteration:
            self.next = None
            return
        _batch_hook(batch)
        n_tok = int((batch[2] - 1).sum())
        with torch.cuda.stream(self.stream):
            imgs = batch[0].to(self.device, non_blocking=True)
            if imgs.dtype != torch.float32:
                imgs = imgs.float()
            caps = batch[1].to(self.device, non_blocking=True)
            caplens = batch[2].to(self.device, non_blocking=True)
            capmasks = batch[3].to(self.device, non_blocking=True)
            ent = batch[4].to(self.device, non_blocking=True)            # the fused step reads them on the device
            facts = batch[6].to(self.device, non_blocking=True) if self.has_facts else None
            ev = torch.cuda.Event()
            ev.record(self.stream)
        if self.release is not None and batch[0].is_pinned():
            self.release[batch[0].data_ptr()] = ev     # the loader's ring may reuse this block once the copy has run
        self.next = ((imgs, caps, caplens, capmasks, ent, facts), n_tok, ev, batch)   # batch: keeps the pinned source alive

    def __iter__(self):
        return self

    def __next__(self):
        if self.next is None:
            raise StopIteration
        tensors, n_tok, ev, _ = self.next
        cur = torch.cuda.current_stream()
        cur.wait_event(ev)
        for t in tensors:
            if t is not None:
                t.record_stream(cur)
        self._load()
        return tensors, n_tok


def make_criteria(pad_token, label_smoothing=0.0):
    """(training criterion, validation criterion) of the unfused path: the training loss carries Config.label_smoothing,
    validation is always the plain negative log-likelihood."""
    return (nn.CrossEntropyLoss(ignore_index=pad_token, label_smoothing=float(label_smoothing)),
            nn.CrossEntropyLoss(ignore_index=pad_token))


def packed_loss(criterion, scores, caps_sorted, decode_lengths):
    targets = caps_sorted[:, 1:]
    s = pack_padded_sequence(scores, decode_lengths, batch_first=True).data
    t = pack_padded_sequence(targets, decode_lengths, batch_first=True).data
    return criterion(s, t)


class TorchEma:
    """The unfused path's moving average of the trained parameters: the definition TrainStep(ema_decay=) follows, as a
    plain lerp_ per parameter after optimizer.step().  The same state layout as TrainStep.ema_state_dict(): "params" for
    the decoder optimizer's parameters in its order, "encoder_params" for the encoder optimizer's (fine_tune_encoder)."""

    def __init__(self, decay, warmup, decoder_optimizer, encoder_optimizer=None):
        self.decay, self.warmup = check_ema_decay(decay), bool(warmup)
        groups = lambda opt: [p for g in opt.param_groups for p in g["params"]] if opt is not None else []     # noqa: E731
        self.params, self.enc_params = groups(decoder_optimizer), groups(encoder_optimizer)
        self.avg = [p.detach().clone() for p in self.params + self.enc_params]

    def update(self, t):
        """After the t-th (1-based) optimizer step."""
        w = 1.0 - ema_decay_at(t, self.decay, self.warmup)
        with torch.no_grad():
            for e, p in zip(self.avg, self.params + self.enc_params):
                e.lerp_(p.detach(), w)

    def state_dict(self):
        n = len(self.params)
        sd = {"decay": self.decay, "warmup": self.warmup, "params": [e.clone() for e in self.avg[:n]]}
        if self.enc_params:
            sd["encoder_params"] = [e.clone() for e in self.avg[n:]]
        return sd

    def load_state_dict(self, sd):
        theirs = list(sd["params"]) + list(sd.get("encoder_params", ()))
        if len(sd["params"]) != len(self.params) or len(theirs) != len(self.avg) or \
                any(tuple(t.shape) != tuple(e.shape) for t, e in zip(theirs, self.avg)):
            raise ValueError("the checkpoint's moving average does not fit the trained parameters")
        with torch.no_grad():
            for e, t in zip(self.avg, theirs):
                e.copy_(t)

    @contextlib.contextmanager
    def weights(self):
        """Inside: the parameters hold the averages (exchanged, and exchanged back on the way out)."""
        def exchange():
            with torch.no_grad():
                for e, p in zip(self.avg, self.params + self.enc_params):
                    t = p.detach().clone()
                    p.copy_(e)
                    e.copy_(t)
        exchange()
        try:
            yield self
        finally:
            exchange()


def train(loader, encoder, decoder, criterion, decoder_optimizer, step, epoch, cfg, device, encoder_optimizer=None,
          ema=None):
    decoder.train()
    encoder.train()
    batch_time, losses = ut.AverageMeter(), ut.AverageMeter()
    has_facts = decoder.has_facts
    start = t_epoch = time.time()
    if step is not None and cfg.prefetch:
        return _train_fused_pipelined(loader, encoder, step, epoch, cfg, device, has_facts)
    n_steps = 0
    for i, batch in enumerate(loader):
        n_steps = i + 1
        imgs, caps, caplens, capmasks, ent, facts = _batch_to_device(batch, device, has_facts)
        extra = (facts,) if has_facts else ()
        if encoder_optimizer is not None:
            enc = encoder(imgs)                     # fine_tune_encoder: the loss back-propagates into the encoder
        elif step is not None and step.train_conv1:
            enc = None                              # the step projects the feature map itself
        else:
            with torch.no_grad():
                enc = encoder(imgs)
        n_tok = int((caplens - 1).sum())
        if step is not None:                                             # fused HIP step
            # (train_conv1: the step runs Encoder.conv1 itself and needs the feature map to train it)
            loss = step(caps, imgs if step.train_conv1 else enc, capmasks, caplens, ent, *extra).item()
        else:                                                            # the reference's statement sequence
            scores, caps_sorted, dl = decoder(caps, enc, capmasks, caplens, ent, *extra)
            loss_t = packed_loss(criterion, scores, caps_sorted, dl)
            decoder_optimizer.zero_grad()
            if encoder_optimizer is not None:
                encoder_optimizer.zero_grad()
            loss_t.backward()
            if cfg.max_grad_norm is not None:
                STATS["last_grad_norm"] = torch.nn.utils.clip_grad_norm_(
                    [p for g in decoder_optimizer.param_groups for p in g["params"]], cfg.max_grad_norm)
            if cfg.lr_schedule is not None:
                _set_scheduled_lr(decoder_optimizer, cfg.lr_schedule)
            if cfg.grad_clip is not None:
                ut.clip_gradient(decoder_optimizer, cfg.grad_clip)
                if encoder_optimizer is not None:
                    ut.clip_gradient(encoder_optimizer, cfg.grad_clip)
            decoder_optimizer.step()
            if encoder_optimizer is not None:
                encoder_optimizer.step()
            if ema is not None:
                ema.update(_optimizer_steps(decoder_optimizer))
            loss = loss_t.item()
        losses.update(loss, n_tok)
        batch_time.update(time.time() - start)
        start = time.time()
        if i % cfg.print_freq == 0:
            print("Epoch: [%d][%d/%d]\tBatch Time %.3f (%.3f)\tLoss %.4f (%.4f)" %
                  (epoch, i, len(loader), batch_time.val, batch_time.avg, losses.val, losses.avg))
        if cfg.max_batches and i + 1 >= cfg.max_batches:
            break
    STATS["last_epoch_steps_per_s"] = n_steps / max(time.time() - t_epoch, 1e-9)
    return losses.avg


def _has_decay_groups(opt):
    return len(opt.param_groups) > 1 or any(g.get("weight_decay", 0) != 0 for g in opt.param_groups)


def make_decoder_optimizer(decoder, cfg, old=None):
    """The unfused path's decoder optimizer.  Without cfg.weight_decay torch.optim.Adam over the trainable parameters, as
    ever; with it AdamW (or Adam, decoupled_weight_decay=False) over ONE PARAM GROUP PER PARAMETER in the same order, the
    decay on the parameters training.default_decay_filter selects -- the layout TrainStep.state_dict() reports.  old: a
    resumed optimizer; its moments, step counts, rate, betas and eps carry over (parameter i of its flattened groups is
    parameter i here), its decay does not: that comes from cfg."""
    named = [(n, p) for n, p in decoder.named_parameters() if p.requires_grad]
    if cfg.weight_decay is None:
        opt = torch.optim.Adam([p for _, p in named], lr=cfg.decoder_lr)
    else:
        cls = torch.optim.AdamW if cfg.decoupled_weight_decay else torch.optim.Adam
        opt = cls([dict(params=[p], weight_decay=float(cfg.weight_decay) if default_decay_filter(n, p) else 0.0)
                   for n, p in named], lr=cfg.decoder_lr, weight_decay=0.0)
    if old is not None:
        theirs, mine = old.state_dict(), opt.state_dict()
        ids = [i for g in theirs["param_groups"] for i in g["params"]]
        if len(ids) != len(named):
            raise ValueError("the checkpoint's decoder_optimizer holds %d parameters, the decoder trains %d"
                             % (len(ids), len(named)))
        keep = {k: v for k, v in theirs["param_groups"][0].items() if k in ("lr", "base_lr", "betas", "eps")}
        for g in mine["param_groups"]:
            g.update(keep)
        mine["state"] = {k: theirs["state"][i] for k, i in enumerate(ids) if i in theirs["state"]}
        opt.load_state_dict(mine)
    return opt


def _optimizer_steps(opt):
    """Steps a torch Adam has taken (every parameter of ours steps together; 0 before the first)."""
    for st in opt.state.values():
        if "step" in st:
            return int(float(st["step"]))
    return 0


def _set_scheduled_lr(opt, schedule):
    """Unfused path: the rate of the optimizer step about to be taken, from the group's base rate (kept beside "lr" under
    "base_lr", which the plateau decay multiplies and a checkpoint carries) and training.lr_at."""
    t = _optimizer_steps(opt) + 1
    for g in opt.param_groups:
        g["lr"] = lr_at(t, g.setdefault("base_lr", g["lr"]), schedule)


def _train_fused_pipelined(loader, encoder, step, epoch, cfg, device, has_facts):
    """The fused step fed by the Prefetcher: no host synchronisation inside the loop except when a line is printed --
    the token-weighted loss sum stays on the device until the epoch ends.  When the step owns the (frozen) encoder it
    takes the feature map itself and Encoder.conv1 runs inside the captured step."""
    loss_sum = torch.zeros(1, device=device)
    tok_sum, start, t_epoch = 0, time.time(), time.time()
    n = 0
    for i, (tensors, n_tok) in enumerate(Prefetcher(loader, device, has_facts)):
        imgs, caps, caplens, capmasks, ent, facts = tensors
        extra = (facts,) if has_facts else ()
        if step.enc is not None and imgs.dim() == 4 and imgs.shape[1] == step.enc.encoder_dim:
            loss = step(caps, imgs, capmasks, caplens, ent, *extra)
        else:
            with torch.no_grad():
                enc = encoder(imgs)
            loss = step(caps, enc, capmasks, caplens, ent, *extra)
        loss_sum += loss * float(n_tok)
        tok_sum += n_tok
        n = i + 1
        if i % cfg.print_freq == 0:
            now = time.time()
            print("Epoch: [%d][%d/%d]\tBatch Time %.3f\tLoss %.4f (%.4f)" %
                  (epoch, i, len(loader), now - start, loss.item(), loss_sum.item() / max(tok_sum, 1)))
        start = time.time()
        if cfg.max_batches and i + 1 >= cfg.max_batches:
            break
    step.flush()                                       # (lazy_update) the last step's optimizer update, before validation
    avg = loss_sum.item() / max(tok_sum, 1)            # the epoch's one synchronisation
    STATS["last_epoch_steps_per_s"] = n / max(time.time() - t_epoch, 1e-9)
    return avg


def _train_scst(loader, encoder, sc, epoch, cfg, device, has_facts):
    """One SCST epoch: the plain fused loop (batches moved synchronously, no prefetch pipeline); each batch's captions
    are its references.  The host waits only when a line is printed (mean sample and greedy CIDEr-D of that batch,
    also kept in STATS["scst_rewards"]).  Returns the mean weighted loss."""
    loss_sum = torch.zeros(1, device=device)
    n, t_epoch = 0, time.time()
    for i, batch in enumerate(loader):
        imgs, caps, caplens, capmasks, ent, facts = _batch_to_device(batch, device, has_facts)
        with torch.no_grad():
            enc = encoder(imgs)
        out = sc(enc, ent, facts, refs=caps)
        loss_sum += out.loss
        n = i + 1
        if i % cfg.print_freq == 0:
            r_s = out.rewards.mean().item()
            r_g = out.greedy_rewards.mean().item() if out.greedy_rewards is not None else float("nan")
            STATS.setdefault("scst_rewards", []).append((epoch, i, r_s, r_g))
            print("Epoch: [%d][%d/%d]\tSCST loss %.4f\t%s sample %.4f greedy %.4f" %
                  (epoch, i, len(loader), out.loss.item(), "CIDEr-D" if cfg.scst_reward is None else "reward", r_s, r_g))
        if cfg.max_batches and i + 1 >= cfg.max_batches:
            break
    STATS["last_epoch_steps_per_s"] = n / max(time.time() - t_epoch, 1e-9)
    return loss_sum.item() / max(n, 1)


class _ValCaptionMetrics:
    """Config.val_caption_metrics: the greedy captions of every validation batch, scored against the batch's caption rows
    (one reference per image in this dataset format).  Per batch one decode, one ick_caption_metrics launch, one totals
    launch and a device add; finish() reads the totals -- the pass's one extra synchronisation."""

    def __init__(self, decoder, device, cider=None, geo=None):
        self.dec, self.cider = decoder, cider
        self.geo = GeoReferenceMetric(decoder.word_map, device=device, **geo) if geo is not None else None
        self.geo_counts, self.rows = None, 0
        self.metrics = CaptionMetrics(decoder.word_map, pointer_base=decoder.vocab_size, device=device)
        self.totals = None
        self.cider_sum = torch.zeros(1, device=device, dtype=torch.float64) if cider is not None else None

    def add(self, enc, caps, ent, facts, names=None):
        seq = self.dec.predict(enc, caps.shape[1], ent, *((facts,) if facts is not None else ()))
        rows = seq.t().contiguous()
        idx = torch.arange(rows.shape[0], device=rows.device, dtype=torch.int32)
        t = self.metrics.totals(self.metrics(rows, idx, caps))
        self.totals = t if self.totals is None else self.totals + t
        if self.cider is not None:
            self.cider_sum += self.cider(rows, idx, caps).double().sum()
        if self.geo is not None:
            c = self.geo(rows, idx, ent, names, row_offset=self.rows)
            self.geo_counts = c if self.geo_counts is None else self.geo_counts + c
            self.rows += rows.shape[0]

    def finish(self):
        if self.totals is None:
            return {}
        tensors = list(self.totals) + ([self.cider_sum] if self.cider is not None else [])
        if self.geo is not None:
            tensors += [self.geo_counts.generated, self.geo_counts.random]
        if dp.world_size() > 1:                                 # every rank scored its own shard
            for t in tensors:
                torch.distributed.all_reduce(t)
        res = CaptionMetrics.result(self.totals)
        if self.cider is not None:
            res["CIDEr-D"] = float(self.cider_sum.item()) / max(res["captions"], 1)
        STATS["caption_metrics"] = res
        print("Validation: " + "\t".join("%s %.4f" % (k, v) for k, v in res.items() if k != "captions")
              + " (%d captions)" % res["captions"])
        if self.geo is not None:
            res["geo_js"] = self.geo.result(self.geo_counts)
            for name, terms in res["geo_js"].items():
                print("Validation: geo references, %s: " % name + "\t".join(
                    "%s %d" % (t, v["n_occurrences"]) + "".join(" %s %.4f" % (f, x) for f, x in v.items()
                                                                if f != "n_occurrences" and x is not None)
                    for t, v in terms.items()))
        return res


def validate(loader, encoder, decoder, criterion, cfg, device, cider=None):
    """Token-weighted mean loss over the validation split (geo-aware/train.py:317-386).  Under torchrun every rank
    scores its own shard and the (sum, count) pair is all-reduced, so all ranks return the same number and take the
    same best-checkpoint / lr-decay / early-stop decisions.  With Config.val_caption_metrics it returns (loss, the
    caption metrics of the greedy captions as a dict); cider: a CiderD whose corpus score joins that dict."""
    decoder.eval()
    encoder.eval()
    cm = _ValCaptionMetrics(decoder, device, cider, cfg.val_geo_metric) if cfg.val_caption_metrics else None
    if cfg.val_token_metrics:
        loss = _validate_token_metrics(loader, encoder, decoder, cfg, device, cm)
        return (loss, cm.finish()) if cm is not None else loss
    losses = ut.AverageMeter()
    has_facts = decoder.has_facts
    with torch.no_grad():
        for i, batch in enumerate(loader):
            imgs, caps, caplens, capmasks, ent, facts = _batch_to_device(batch, device, has_facts)
            extra = (facts,) if has_facts else ()
            enc = encoder(imgs)
            scores, caps_sorted, dl = decoder(caps, enc, capmasks, caplens, ent, *extra)
            losses.update(packed_loss(criterion, scores, caps_sorted, dl).item(), sum(dl))
            if cm is not None:
                cm.add(enc, caps, ent, facts, batch[5])
            if cfg.max_batches and i + 1 >= cfg.max_batches:
                break
    total, count = dp.reduce_sum_count(losses.sum, losses.count, device=device)
    loss = total / max(count, 1.0)
    return (loss, cm.finish()) if cm is not None else loss


def _validate_token_metrics(loader, encoder, decoder, cfg, device, cm=None):
    """validate() with Config.val_token_metrics: every batch goes through decoder.score_captions (the score head over the
    valid positions only, no (B, L, V+K+F) matrix, no per-batch .item()); the four totals are accumulated on the device
    and read once at the end.  Same token-weighted loss; also prints and records perplexity and top-1 / top-5 accuracy."""
    acc = torch.zeros(4, device=device, dtype=torch.float64)
    with torch.no_grad():
        for i, batch in enumerate(loader):
            imgs, caps, caplens, capmasks, ent, facts = _batch_to_device(batch, device, decoder.has_facts)
            enc = encoder(imgs)
            s = decoder.score_captions(caps, enc, capmasks, caplens, ent, facts, top_k=5)
            acc += torch.cat([s.loss_sum, s.count, s.top1_hits, s.topk_hits]).double()
            if cm is not None:
                cm.add(enc, caps, ent, facts, batch[5])
            if cfg.max_batches and i + 1 >= cfg.max_batches:
                break
    loss_sum, count, top1, top5 = acc.tolist()                  # the one synchronisation
    total, count = dp.reduce_sum_count(loss_sum, count, device=device)
    top1, top5 = dp.reduce_sum_count(top1, top5, device=device)
    loss = total / max(count, 1.0)
    STATS["val_perplexity"] = math.exp(loss) if loss < 700.0 else float("inf")
    STATS["val_top1"], STATS["val_top5"] = top1 / max(count, 1.0), top5 / max(count, 1.0)
    print("Validation: perplexity %.3f\ttop-1 accuracy %.4f\ttop-5 accuracy %.4f (%d tokens)"
          % (STATS["val_perplexity"], STATS["val_top1"], STATS["val_top5"], int(count)))
    return loss


class ShardSampler(torch.utils.data.Sampler):
    """Rank r of w takes every w-th index of the split, in order, WITHOUT padding (validation: no sample may be
    counted twice; the shards may differ in length by one because no collective runs inside the loop)."""

    def __init__(self, n, rank, world):
        self.idx = list(range(rank, n, world))

    def __iter__(self):
        return iter(self.idx)

    def __len__(self):
        return len(self.idx)


def make_loaders(cfg, rank, world, fused=None):
    """TRAIN: one permutation per epoch shared by all ranks (seed + epoch), dealt out in disjoint equal shards --
    DistributedSampler pads by wrapping around so that every rank runs the same number of steps (each step holds a
    collective).  The global batch is cfg.batch_size * world samples.  VAL: disjoint unpadded shards."""
    fused = cfg.fused if fused is None else fused       # main(): fine_tune_encoder turns the fused step off
    data = {s: CaptionDataset(cfg.data_dir, cfg.data_name, s, keep_half=cfg.half_features and fused and cfg.prefetch
                              and s == "TRAIN") for s in ("TRAIN", "VAL")}
    samplers = {"TRAIN": None, "VAL": None}
    if world > 1:
        samplers["TRAIN"] = torch.utils.data.distributed.DistributedSampler(
            data["TRAIN"], num_replicas=world, rank=rank, shuffle=True, seed=cfg.seed, drop_last=False)
        samplers["VAL"] = ShardSampler(len(data["VAL"]), rank, world)
    gen = torch.Generator()
    gen.manual_seed(cfg.seed)
    def loader(split, shuffle):
        ds, smp = data[split], samplers[split]
        if ds.precomputed and ds.transform is None:
            # whole batches: ds[[indices]] builds the batch in one go (datasets.CaptionDataset.fetch_batch)
            base = smp if smp is not None else (torch.utils.data.RandomSampler(ds, generator=gen) if shuffle
                                                else torch.utils.data.SequentialSampler(ds))
            bs = torch.utils.data.BatchSampler(base, cfg.batch_size, drop_last=False)
            if split == "TRAIN" and cfg.loader_threads > 0:
                return ThreadedBatches(ds, bs, cfg.loader_threads)
            return torch.utils.data.DataLoader(ds, sampler=bs, batch_size=None, num_workers=cfg.workers, pin_memory=True)
        return torch.utils.data.DataLoader(ds, batch_size=cfg.batch_size, shuffle=shuffle and smp is None, sampler=smp,
                                           num_workers=cfg.workers, pin_memory=True, generator=gen if shuffle else None)

    loaders = {"TRAIN": loader("TRAIN", True), "VAL": loader("VAL", False)}
    return loaders, samplers, gen


def _bucket_range(step):
    return (step.flat_p.data_ptr(), step.flat_p.data_ptr() + 4 * step.flat_p.numel())


def main(cfg=None):
    cfg = cfg or Config()
    world = dp.init_from_env()
    rank = int(os.environ.get("RANK", "0"))
    if world > 1 and (not cfg.fused or cfg.fine_tune_encoder):
        raise ValueError("data-parallel training needs fused=True and fine_tune_encoder=False (TrainStep owns the "
                         "gradient all-reduce; the encoder's gradients are not part of its bucket)")
    if cfg.train_conv1 and (cfg.fine_tune_encoder or cfg.scst or not cfg.fused):
        raise ValueError("train_conv1=True trains Encoder.conv1 inside the fused step: it needs fused=True and excludes "
                         "fine_tune_encoder=True (the unfused way to train the encoder) and scst=True (its samples reach "
                         "the step as token-major encoder rows)")
    fused = cfg.fused and not cfg.fine_tune_encoder     # fine-tuning the encoder takes the reference's statement
                                                        # sequence: loss.backward() through the HIP autograd bridge
    if cfg.scst and (not fused or world > 1 or cfg.scst_baseline not in ("greedy", "mean")):
        raise ValueError('scst=True needs a fused single-process run (fused=True, fine_tune_encoder=False, no torchrun) '
                         'and scst_baseline "greedy" or "mean"')
    if cfg.val_geo_metric is not None and not (cfg.val_caption_metrics and isinstance(cfg.val_geo_metric, dict)):
        raise ValueError("val_geo_metric is a dict of GeoReferenceMetric's arguments and rides on val_caption_metrics=True "
                         "(the pass that decodes the validation batches)")
    if cfg.scst_reward is not None and not (cfg.scst and isinstance(cfg.scst_reward, dict) and
                                            "cider" not in cfg.scst_reward):
        raise ValueError("scst_reward is a dict of CaptionMetrics.reward()'s keyword arguments without `cider`, and "
                         "needs scst=True")
    device = torch.device("cuda", int(os.environ.get("LOCAL_RANK", "0")) % max(1, torch.cuda.device_count()))
    torch.cuda.set_device(device)
    models = load_models(cfg.variant)
    with open(os.path.join(cfg.data_dir, "WORDMAP_" + cfg.data_name + ".json")) as f:
        word_map = json.load(f)
    best_loss, epochs_since_improvement, start_epoch = 1e5, 0, cfg.start_epoch
    if not cfg.checkpoint:
        decoder = models.DecoderTransformer(word_map=word_map, emb_dim=cfg.emb_dim, decoder_dim=cfg.decoder_dim,
                                            encoder_dim=cfg.encoder_dim, num_heads=cfg.num_heads,
                                            num_layers=cfg.num_layers)
        if cfg.pretrained_word_embeddings_file:
            decoder.load_pretrained_embeddings(ut.load_embeddings(cfg.pretrained_word_embeddings_file, word_map))
        decoder.fine_tune_embeddings(True)
        # fine-tuning needs the trunk's parameters to exist before encoder.fine_tune() and the encoder optimizer see them
        # (a trunk built lazily by the first raw-image batch would be missing from the optimizer)
        encoder = models.Encoder(emb_dim=cfg.emb_dim, with_trunk=True if cfg.fine_tune_encoder else None)
        decoder_optimizer = encoder_optimizer = None
    else:
        ck = ut.load_checkpoint(cfg.checkpoint, map_location=device)
        decoder, encoder = ck["decoder"], ck["encoder"]
        decoder_optimizer = None if cfg.zero_out_epochs_since_improvement else ck["decoder_optimizer"]
        encoder_optimizer = None if cfg.zero_out_epochs_since_improvement else ck.get("encoder_optimizer")
        if not cfg.zero_out_epochs_since_improvement:
            start_epoch, epochs_since_improvement, best_loss = ck["epoch"] + 1, ck["epochs_since_improvement"], ck["loss"]
    decoder.to(device)
    encoder.to(device)
    if cfg.fine_tune_encoder and "resnet" not in encoder._modules:      # e.g. a checkpoint saved without the trunk
        encoder._build_trunk()
    encoder.fine_tune(cfg.fine_tune_encoder)
    if cfg.fine_tune_encoder and encoder_optimizer is None:
        encoder_optimizer = torch.optim.Adam([p for p in encoder.parameters() if p.requires_grad], lr=cfg.encoder_lr)
    encoder_optimizer_ck = encoder_optimizer            # train_conv1: the step takes its state over below
    if not cfg.fine_tune_encoder:
        encoder_optimizer = None
    step = None
    if fused:
        # seed: the dropout stream, one per rank (the ranks hold different samples); the constructor broadcasts rank
        # 0's weights, so a decoder that was randomly initialised per process starts identical everywhere
        # encoder=: with the frozen encoder the step takes the feature map itself (Encoder.conv1 inside the captured step)
        det = cfg.deterministic
        if det is None and os.environ.get("ICK_DETERMINISTIC") is not None:
            det = os.environ["ICK_DETERMINISTIC"] not in ("", "0")      # the script's switch, read when main() runs
        pipelined = cfg.prefetch and not cfg.scst
        step = TrainStep(decoder, lr=cfg.decoder_lr, grad_clip=cfg.grad_clip, seed=cfg.seed * 1000 + rank,
                         encoder=encoder if pipelined or cfg.train_conv1 else None, deterministic=det,
                         train_conv1=cfg.train_conv1, encoder_lr=cfg.encoder_lr,
                         # the pipelined loop lets step i's optimizer update run at the head of step i + 1's graph beside
                         # Encoder.conv1; _train_fused_pipelined() flushes the last one of an epoch
                         lazy_update=bool(pipelined), label_smoothing=cfg.label_smoothing,
                         max_grad_norm=cfg.max_grad_norm, lr_schedule=cfg.lr_schedule, ema_decay=cfg.ema_decay,
                         ema_warmup=cfg.ema_warmup, weight_decay=cfg.weight_decay,
                         decoupled_weight_decay=cfg.decoupled_weight_decay, encoder_weight_decay=cfg.encoder_weight_decay,
                         # (seed None: the step's own, which is offset by the rank above; the probability is set per epoch)
                         scheduled_sampling=None if cfg.scheduled_sampling_start < 0 else
                         dict(prob=0.0, mode=cfg.scheduled_sampling_mode))
        if decoder_optimizer is not None:
            # resume: Adam moments, step count (bias correction + dropout stream position) and the decayed lr come
            # back from the pickled optimizer (ours or one written by the reference, geo-aware/utils.py:32-46)
            step.load_state_dict(decoder_optimizer.state_dict())
            decoder_optimizer = None
        if cfg.train_conv1 and encoder_optimizer_ck is not None:
            step.load_encoder_state_dict(encoder_optimizer_ck.state_dict())     # (after the decoder's: it sets the step count)
        # what the bucket does not cover (frozen Encoder.conv1 and trunk, frozen decoder parameters, buffers) also
        # starts from rank 0's copy: every process initialised its own
        dp.broadcast_module_state([encoder, decoder], _bucket_range(step))
    elif decoder_optimizer is None:
        decoder_optimizer = make_decoder_optimizer(decoder, cfg)
    elif cfg.weight_decay is not None or _has_decay_groups(decoder_optimizer):
        # resume across decay on / off: the moments carry over, the decay and the group layout come from the Config
        decoder_optimizer = make_decoder_optimizer(decoder, cfg, old=decoder_optimizer)
    # the moving average: the fused step keeps its own; the unfused path's is a lerp_ after optimizer.step().  A resumed
    # run takes it from the checkpoint (a checkpoint without one: the average starts at the loaded weights).
    ema = None
    if cfg.ema_decay is not None:
        if step is None:
            ema = TorchEma(cfg.ema_decay, cfg.ema_warmup, decoder_optimizer, encoder_optimizer)
        ema_ck = ck.get("decoder_ema") if cfg.checkpoint and not cfg.zero_out_epochs_since_improvement else None
        if ema_ck is not None:
            (step.load_ema_state_dict if step is not None else ema.load_state_dict)(
                dict(ema_ck, decay=cfg.ema_decay, warmup=cfg.ema_warmup))
    if step is None:
        check_max_grad_norm(cfg.max_grad_norm)
        check_lr_schedule(cfg.lr_schedule)
    criterion, val_criterion = (c.to(device) for c in make_criteria(word_map["<pad>"], cfg.label_smoothing))
    loaders, samplers, shuffle_gen = make_loaders(cfg, rank, world, fused)
    if cfg.train_conv1 and not loaders["TRAIN"].dataset.precomputed:
        raise ValueError("train_conv1=True needs a dataset of precomputed feature maps: with raw images the ResNet trunk "
                         "runs outside the step (fine_tune_encoder=True trains the encoder there)")
    sc = cider = None
    if cfg.scst:
        captions = torch.as_tensor(np.asarray(loaders["TRAIN"].dataset.captions), dtype=torch.long)
        cider = reward = CiderD(captions, word_map, device=device)
        if cfg.scst_reward is not None:
            reward = CaptionMetrics(word_map, pointer_base=len(word_map), device=device).reward(cider=cider,
                                                                                                **cfg.scst_reward)
        # sampled rows one shorter than the dataset's captions: the training rows ([<start>] + samples) keep its width
        sc = SelfCriticalStep(step, reward, num_samples=cfg.scst_samples, baseline=cfg.scst_baseline,
                              max_len=captions.shape[1] - 1, seed=cfg.seed)
    history = []
    for epoch in range(start_epoch, cfg.epochs):
        if epochs_since_improvement == cfg.max_epochs_since_improvement:
            break
        if epochs_since_improvement > 0 and epochs_since_improvement % 8 == 0:
            if step is not None:
                step.set_lr(step.lr * 0.8)
            else:
                ut.adjust_learning_rate(decoder_optimizer, 0.8)
                for g in decoder_optimizer.param_groups:        # (with lr_schedule: the base rate the schedule multiplies)
                    if "base_lr" in g:
                        g["base_lr"] *= 0.8
            if encoder_optimizer is not None:
                ut.adjust_learning_rate(encoder_optimizer, 0.8)
            if step is not None and step.train_conv1:
                step.set_encoder_lr(step.encoder_lr * 0.8)
        # the epoch's permutation depends on (seed, epoch) only, so a resumed run sees the batches the interrupted
        # one would have seen
        shuffle_gen.manual_seed(cfg.seed * 100003 + epoch)
        if step is not None and step.ss is not None:
            step.set_sampling_prob(sampling_prob_at(epoch, cfg.scheduled_sampling_start, cfg.scheduled_sampling_increase_every,
                                                    cfg.scheduled_sampling_increase_prob, cfg.scheduled_sampling_max_prob))
            STATS["sampling_prob"] = step.ss["prob"]
        if samplers["TRAIN"] is not None:
            samplers["TRAIN"].set_epoch(epoch)
        if sc is not None:
            tr = _train_scst(loaders["TRAIN"], encoder, sc, epoch, cfg, device, decoder.has_facts)
        else:
            tr = train(loaders["TRAIN"], encoder, decoder, criterion, decoder_optimizer, step, epoch, cfg, device,
                       encoder_optimizer, ema)
        if cfg.max_grad_norm is not None:
            # one read per epoch: the norm of the last update (the fused step keeps it in a device word)
            norm = float(step.grad_norm.item() if step is not None else STATS.get("last_grad_norm", float("nan")))
            STATS["last_grad_norm"] = norm
            if rank == 0:
                print("Epoch: [%d]\tgradient norm of the last step %.4f (max_grad_norm %g)" % (epoch, norm, cfg.max_grad_norm))
        averaged = contextlib.nullcontext()
        if cfg.ema_decay is not None and cfg.ema_validate:      # early stopping and BEST_ then follow the averaged weights
            averaged = step.ema_weights() if step is not None else ema.weights()
        with averaged:
            last_loss = validate(loaders["VAL"], encoder, decoder, val_criterion, cfg, device, cider=cider)   # identical on every rank
        if cfg.val_caption_metrics:
            last_loss = last_loss[0]                    # (the metrics dict is printed and kept in STATS)
        is_best = last_loss < best_loss
        best_loss = min(last_loss, best_loss)
        epochs_since_improvement = 0 if is_best else epochs_since_improvement + 1
        history.append((tr, last_loss))
        if step is not None and world > 1 and not (dp.replicas_agree(step.flat_p) and
                                                   dp.module_state_agrees([encoder, decoder], _bucket_range(step))):
            raise RuntimeError("data-parallel replicas diverged (epoch %d): parameters differ between ranks" % epoch)
        if rank == 0:
            opt = step.as_torch_optimizer() if step is not None else decoder_optimizer
            enc_opt = step.as_torch_encoder_optimizer() if step is not None and step.train_conv1 else encoder_optimizer
            extra = {}
            if cfg.ema_decay is not None:
                extra["decoder_ema"] = (step.ema_state_dict() if step is not None else ema.state_dict())
            ut.save_checkpoint(cfg.data_name, epoch, epochs_since_improvement, encoder, decoder, enc_opt,
                               opt, last_loss, is_best, out_dir=cfg.out_dir, **extra)
    return history


if __name__ == "__main__":
    main()
