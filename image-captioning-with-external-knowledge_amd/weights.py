"""Re-laid-out copies of the decoder's weights.  Every fast path reads the
weights through such copies; WeightImages owns all of them -- one object per decoder, the only code that allocates or fills
one -- and DerivedWeights is the table that lets the optimizer kernel (ick_adam_step_derive, csrc/adam.hip) write
them in the same pass as the update: the reference's optimizer.step() (geo-aware/train.py:292) is the only writer of the
parameters, so nothing has to re-pack a weight in front of the next forward pass."""
import weakref

import torch

from . import ops
from .lib import IckError


def first_stage(key):
    """The chain images a captured training step packs first: the context encoders' and layer 0's self block's."""
    return key[0] != "d" or (key[1] == 0 and key[2] in ("so", "cq", "si"))


def vocab_planes_wanted(rows):
    """The vocabulary GEMM reads fc_vocab's bf16 planes from 256 rows on; below it runs on the plain weight."""
    return rows >= 256


class _Image:
    """One table entry: `kind` ("pack" | "copy" | "presplit") of the 2-D view `view(*parameters)`.  params: (module,
    attribute name) pairs, read from the live module on every use; out: a copy's (buffer name, buffer shape, first row, end
    row) inside the group; of_image: the view is of the kv group's image (WeightImages.NEEDS); dst: set on allocation."""

    def __init__(self, group, key, kind, params, view, out=None, of_image=False):
        self.group, self.key, self.kind, self.params, self.view, self.out = group, key, kind, params, view, out
        self.of_image, self.dst = of_image, None

    def src(self, owner):
        return self.view(owner.wkv) if self.of_image else self.view(*[getattr(m, a).detach() for m, a in self.params])


class WeightImages:
    """Every re-laid-out copy of a decoder's weights, in persistent buffers, by group:

      kv          rows [d:3d] of every decoder layer's cross-attention in_proj gathered into one (2 * layers * d, d) weight
                  and bias (one GEMM projects the memory for all layers)
      kv_ps       bf16 hi / mid / lo planes of that weight (csrc/gemm_ps.hip's B operand)
      vocab_ps / vocab_t_ps     the planes of fc_vocab.weight and of its transpose (forward, data gradient)
      pred_wt     fc_predicate.weight transposed (knowledge / news variants)
      chain       packed row-chain images of every nn.Linear a chain launch (ops.rowchain_fwd) multiplies with
      chain_t     the same of the transposed weights (ops.rowchain_bwd) and of the transposed kv weight, ("kv", "T")
      decode      out_proj / out_proj / linear2 of every decoder layer transposed, for the fused decode kernels

    A group is allocated when first asked for -- never inside a stream capture -- and never again: captured graphs and
    the optimizer kernel's table hold the addresses.  The object belongs to the parameter storage it was built from;
    DecoderTransformer.weight_images() replaces it (and the graphs that read it) when a parameter has moved.  A group is
    stale when its stamp differs from key(): _param_epoch (invalidate_caches) + its parameters' version counters."""

    GROUPS = ("kv", "kv_ps", "vocab_ps", "vocab_t_ps", "pred_wt", "chain", "chain_t", "decode")
    NEEDS = {"kv_ps": "kv", "chain_t": "kv"}      # groups with an image made from the kv group's weight

    def __init__(self, dec):
        self._dec = weakref.ref(dec)      # (the decoder holds this object; nothing in the table refers back to it: no cycle)
        self.groups = {g: [] for g in self.GROUPS}
        for e in self._table(dec):
            self.groups[e.group].append(e)
        self.sources = {g: list(dict.fromkeys(p for e in es for p in e.params)) for g, es in self.groups.items()}
        self._all = list(dict.fromkeys(p for ps in self.sources.values() for p in ps))
        self.pointers = self._pointers()
        self.img, self.flat, self.stamp = {}, {}, {}

    def _table(self, dec):
        """The images, from the module tree.  chain keys: per layer the self-attention out-projection "so", the
        cross-attention q-projection "cq" and out-projection "co", "l1", "l2" and -- from a stack's second layer on -- the
        self-attention in_proj "si", which rides on the previous layer's linear2 + norm launch (layer 0's is a plain GEMM)."""
        d = dec.emb_dim
        layers = list(dec.transformer_decoder.layers)
        rows = 2 * d * len(layers)
        whole, t = (lambda w: w), (lambda w: w.t())
        table = []
        add = lambda *a, **kw: table.append(_Image(*a, **kw))
        kv_w = [(l.multihead_attn, "in_proj_weight") for l in layers]
        for i, l in enumerate(layers):
            lo, hi = 2 * d * i, 2 * d * (i + 1)
            add("kv", ("w", i), "copy", [kv_w[i]], lambda w: w[d:], out=("wkv", (rows, d), lo, hi))
            add("kv", ("b", i), "copy", [(l.multihead_attn, "in_proj_bias")], lambda b: b[d:].view(1, -1),
                out=("bkv", (rows,), lo, hi))
        add("kv_ps", "wkv", "presplit", kv_w, whole, of_image=True)
        add("vocab_ps", "vocab", "presplit", [(dec.fc_vocab, "weight")], whole)
        add("vocab_t_ps", "vocab_t", "presplit", [(dec.fc_vocab, "weight")], t)
        if dec.has_facts:
            w = dec.fc_predicate.weight
            add("pred_wt", "pred_wt", "copy", [(dec.fc_predicate, "weight")], t, out=("pred_wt", (w.shape[1], w.shape[0]), 0, w.shape[1]))
        stacks = [("d", dec.transformer_decoder), ("e", dec.transformer_encoder_entities)]
        if dec.has_facts:
            stacks.append(("f", dec.transformer_encoder_facts))
        for tag, stack in stacks:
            for li, l in enumerate(stack.layers):
                items = [("so", l.self_attn.out_proj, "weight", whole)]
                if tag == "d":
                    items += [("cq", l.multihead_attn, "in_proj_weight", lambda w: w[:d]), ("co", l.multihead_attn.out_proj, "weight", whole)]
                items += [("l1", l.linear1, "weight", whole), ("l2", l.linear2, "weight", whole)]
                if li > 0:
                    items.append(("si", l.self_attn, "in_proj_weight", whole))
                for name, mod, attr, view in items:
                    add("chain", (tag, li, name), "pack", [(mod, attr)], view)
                    add("chain_t", (tag, li, name + "T"), "pack", [(mod, attr)], lambda w, view=view: view(w).t())
        add("chain_t", ("kv", "T"), "pack", kv_w, t, of_image=True)
        for li, l in enumerate(layers):
            for name, mod in (("so", l.self_attn.out_proj), ("co", l.multihead_attn.out_proj), ("l2", l.linear2)):
                n, k = mod.weight.shape
                add("decode", (li, name), "copy", [(mod, "weight")], t, out=((li, name), (k, n), 0, k))
        return table

    def _pointers(self):
        return [(p.data_ptr(), p.device) for p in (getattr(m, a) for m, a in self._all)]

    def matches(self):
        """Do the parameters still live where this object's buffers (and every address handed out) were made for?"""
        return self.pointers == self._pointers()

    def key(self, group):
        return (self._dec().__dict__.get("_param_epoch", 0),) + tuple(getattr(m, a)._version for m, a in self.sources[group])

    def _allocate(self, group):
        dev = self.pointers[0][1]
        if dev.type == "cuda" and torch.cuda.is_current_stream_capturing():
            raise IckError("weight image group %r was first asked for inside a stream capture: allocate in a warm-up run" % group)
        img = self.img[group] = {}
        packs = [e for e in self.groups[group] if e.kind == "pack"]
        if packs:
            sizes = [ops.packed_weight_floats(*e.src(self).shape) for e in packs]
            buf = self.flat[group] = torch.empty(sum(sizes), device=dev, dtype=torch.float32)
            off = 0
            for e, n in zip(packs, sizes):
                e.dst = img[e.key] = buf[off:off + n]
                off += n
        for e in self.groups[group]:
            if e.kind == "presplit":
                e.dst = img[e.key] = ops.presplit_buffer(*e.src(self).shape, dev)
            elif e.kind == "copy":
                name, shape, lo, hi = e.out
                if name not in img:
                    img[name] = torch.empty(shape, device=dev, dtype=torch.float32)
                e.dst = img[name][lo:hi] if len(shape) == 2 else img[name][lo:hi].view(1, -1)

    def request(self, *groups):
        """Allocate the groups (and what they are made from) that are not there yet; their contents stay stale."""
        for g in groups:
            for g_ in (self.NEEDS.get(g), g):
                if g_ is not None and g_ not in self.img:
                    self._allocate(g_)
        return self

    def refresh(self, *groups, subset=None):
        """Fill the groups in place from the live parameters: one ick_pack_weights launch for their packed images and
        plain copies, one ick_presplit_weights launch for their planes, on the current stream (capturable once the groups
        exist).  subset: a predicate on the chain keys; only those images of `chain` / `chain_t` are written, and such a
        group is not stamped.  Only a call that names kv together with chain_t packs twice: ("kv", "T") behind kv's gather."""
        self.request(*groups)
        sel = [e for g in groups for e in self.groups[g]
               if subset is None or g not in ("chain", "chain_t") or subset(e.key)]
        for late in (False, True):
            wave = [e for e in sel if e.kind != "presplit" and (e.of_image and self.NEEDS[e.group] in groups) == late]
            if wave:
                ops.pack_weights([(e.src(self), e.dst) for e in wave if e.kind == "pack"],
                                 [(e.src(self), e.dst) for e in wave if e.kind == "copy"])
        planes = [(e.src(self), e.dst) for e in sel if e.kind == "presplit"]
        if planes:
            ops.presplit_weights(planes)
        for g in groups:
            if subset is None or g not in ("chain", "chain_t"):
                self.stamp[g] = self.key(g)
        return self

    def current(self, *groups):
        """refresh() of those groups (and of what they are made from) whose parameters changed since they were filled."""
        groups = list(dict.fromkeys(g_ for g in groups for g_ in (self.NEEDS.get(g), g) if g_ is not None))
        stale = [g for g in groups if self.stamp.get(g) != self.key(g)]
        if stale:
            self.refresh(*stale)
        return self

    def adopt(self, *groups):
        """Stamp the (allocated) groups as filled from the live parameters without a launch: for the caller that knows
        another writer has just done so -- TrainStep's optimizer kernel, through DerivedWeights -- and is about to run code
        that asks current() for them inside the step (the first pass of scheduled sampling)."""
        for g in groups:
            if g in self.img:
                self.stamp[g] = self.key(g)
        return self

    def planes(self, group, rows=None):
        """The current planes of a presplit group for a GEMM over `rows` rows; None where ick_gemm would not read them
        (the exact fp32 product mode, a vocabulary GEMM below vocab_planes_wanted)."""
        if ops.gemm_split_mode() == 0 or (rows is not None and not vocab_planes_wanted(rows)):
            return None
        return next(iter(self.current(group).img[group].values()))

    # ---- the buffers (allocated groups only) ----
    wkv = property(lambda self: self.img["kv"]["wkv"])
    bkv = property(lambda self: self.img["kv"]["bkv"])
    kv_ps = property(lambda self: self.img["kv_ps"]["wkv"])
    vocab_ps = property(lambda self: self.img["vocab_ps"]["vocab"])
    vocab_t_ps = property(lambda self: self.img["vocab_t_ps"]["vocab_t"])
    pred_wt = property(lambda self: self.img["pred_wt"]["pred_wt"] if self.groups["pred_wt"] else None)
    chain = property(lambda self: self.img["chain"])
    chain_t = property(lambda self: self.img["chain_t"])
    decode = property(lambda self: list(self.img["decode"].values()))


class DerivedWeights:
    """The optimizer kernel's view of a decoder's WeightImages (ops.adam_update(cover=) / ick_adam_step_derive): the item
    table that names, for every trainable weight with an image, where in TrainStep's flat bucket it lives and which buffers
    of the owner its updated values go to, and the block table that covers the bucket.

    build() returns None when the widths do not meet the kernel's alignment rules (include/ick_amd.h); the step then keeps
    the per-step packing launches.  refresh() fills every image from the live parameters with the stand-alone packing
    kernels (first step, after load_state_dict, after a capture's rewound warm-up step, after outside writes)."""

    GROUPS = tuple(g for g in WeightImages.GROUPS if g != "decode")     # the decode kernels' copies are not in the table
    pred_wt = property(lambda self: self.owner.pred_wt)

    @staticmethod
    def build(ts):
        dec = ts.dec
        if not dec.chain_bwd_supported():
            return None
        try:
            return DerivedWeights(ts)
        except _Unsupported:
            return None

    def __init__(self, ts):
        self.dec, self.ts = ts.dec, ts
        self.stale, self._seen = True, None
        self._tables(ts.dec.weight_images())

    def _tables(self, owner):
        """The item and block tables over `owner`'s buffers."""
        from . import lib as L
        ts = self.ts
        self.owner = owner.request(*self.GROUPS)
        dev = ts.flat_p.device
        base, nfl = ts.flat_p.data_ptr(), ts.n

        def where(w):
            """Float offset in the bucket of a (row slice of a) trainable parameter; None for frozen ones (their images are
            filled by refresh() and never change)."""
            off = (w.data_ptr() - base) // 4
            if not (0 <= off and off + w.numel() <= nfl):
                return None
            if w.dim() != 2 or w.stride() != (w.shape[1], 1) or w.shape[1] % 4 or off % 4:
                raise _Unsupported()
            return off

        items, nbytes = [], 0

        def item(w, drow0=0, Nd=None, pack=None, pack_t=None, copy=None, ps=None, ps_t=None, tr=None):
            nonlocal nbytes
            off = where(w)
            if off is None:
                return
            rows, K = w.shape
            if (pack_t is not None and (drow0 % 4 or rows % 4)) or (ps_t is not None and (drow0 % 8 or rows % 8)):
                raise _Unsupported()
            it = L.AdamItem()
            it.off, it.rows, it.K, it.drow0, it.Nd = off, rows, K, drow0, Nd if Nd is not None else rows
            for name, t in (("pack", pack), ("pack_t", pack_t), ("copy", copy), ("ps", ps), ("ps_t", ps_t), ("tr", tr)):
                if t is not None:
                    setattr(it, name, t.data_ptr())
                    nbytes += rows * K * (6 if name in ("ps", "ps_t") else 4)
            if copy is not None:
                it.copy_ld = copy.stride(0)
            if tr is not None:
                it.tr_ld = tr.stride(0)
            items.append(it)

        for e in owner.groups["chain"]:
            item(e.src(owner), pack=e.dst, pack_t=owner.chain_t[e.key[:2] + (e.key[2] + "T",)])
        for e in (e for e in owner.groups["kv"] if e.key[0] == "w"):      # rows [d:3d] of layer i's cross-attention in_proj
            item(e.src(owner), drow0=e.out[2], Nd=e.out[1][0], copy=owner.wkv, ps=owner.kv_ps, pack_t=owner.chain_t[("kv", "T")])
        item(self.dec.fc_vocab.weight.detach(), ps=owner.vocab_ps, ps_t=owner.vocab_t_ps)
        if self.dec.has_facts:
            item(self.dec.fc_predicate.weight.detach(), tr=owner.pred_wt)
        # flat runs that are mirrored into a plain copy: rows [d:3d] of the cross-attention in_proj biases -> bkv
        mirrors = []
        for e in (e for e in owner.groups["kv"] if e.key[0] == "b"):
            b = e.src(owner)
            off = (b.data_ptr() - base) // 4
            if 0 <= off and off + b.numel() <= nfl:
                if off % 4 or b.numel() % 4:
                    raise _Unsupported()
                mirrors.append((off, off + b.numel(), e.dst.data_ptr()))
        # ---- the cover of [0, n): tiles of the items, flat runs of <= 1024 float4 everywhere else
        blocks = []

        def flat(lo, hi, copy=0):
            while lo < hi:
                c = min(4096, hi - lo)
                bl = L.AdamBlock()
                bl.item, bl.cnt4, bl.off4, bl.copy = -1, c // 4, lo // 4, copy
                blocks.append(bl)
                lo += c
                if copy:
                    copy += 4 * c

        cuts = sorted([(it.off, it.off + it.rows * it.K, "item", i) for i, it in enumerate(items)] +
                      [(lo, hi, "mirror", ptr) for lo, hi, ptr in mirrors])
        pos = 0
        for lo, hi, kind, what in cuts:
            if lo < pos:
                raise _Unsupported()       # overlapping views of one parameter
            flat(pos, lo)
            if kind == "mirror":
                flat(lo, hi, what)
            else:
                it = items[what]
                for tn in range(it.drow0 // 64, (it.drow0 + it.rows - 1) // 64 + 1):
                    for tk in range((it.K + 63) // 64):
                        bl = L.AdamBlock()
                        bl.item, bl.tn, bl.tk = what, tn, tk
                        blocks.append(bl)
            pos = hi
        flat(pos, nfl)
        if nfl % 4:
            raise _Unsupported()
        self.n_blocks = len(blocks)
        self.nbytes = 28 * nfl + nbytes      # seven streams of the update + the images' bytes (profiling)

        def upload(structs, typ):
            arr = (typ * max(1, len(structs)))(*structs)
            return torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(dev)

        self.items_dev = upload(items, L.AdamItem)
        self.blocks_dev = upload(blocks, L.AdamBlock)
        self.n_items = len(items)

    def _key(self):
        return tuple(p._version for p in self.ts.params) + (self.dec.__dict__.get("_param_epoch", 0),)

    def mark_current(self):
        """The optimizer kernel has just written every image from the weights it updated."""
        self.stale = False
        self._seen = self._key()

    def ensure_current(self, check=False):
        """check: also walk the parameters' pointers (weight_images()); TrainStep asks for it before it captures."""
        if (self.dec.weight_images() if check else self.dec.__dict__.get("_images")) is not self.owner:
            # the decoder's images were dropped or rebuilt: the tables (and the captured steps) name buffers it no longer reads
            self._tables(self.dec.weight_images())
            self.ts._graphs.clear()
            self.stale = True
        if self.stale or self._seen != self._key():
            self.refresh()

    def refresh(self):
        """Every image from the live parameters, with the stand-alone packing kernels (eager launches on the current stream)."""
        self.owner.refresh(*self.GROUPS)
        self.mark_current()


class _Unsupported(Exception):
    pass
