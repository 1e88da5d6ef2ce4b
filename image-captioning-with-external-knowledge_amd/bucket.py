"""ParamBucket: a list of parameters living in one flat fp32 allocation, with Adam's two moments and an optional moving
average laid out alike.  TrainStep keeps one over the decoder's parameters and, with train_conv1, one over
Encoder.conv1's.  Pure torch: no kernel and no library behind it."""
import torch

ALIGN = 64      # floats (256 bytes): the GEMM's 16-byte vector loads need aligned weight rows, and one odd-sized parameter
                # (fc_entity.bias has a single element) would misalign all that follow


class ParamBucket:
    """p / m / v [/ e]: n floats each, parameter i at offsets[i] (a multiple of ALIGN; the pads stay zero); the parameters
    themselves become views of p.  The gradients live in the owner's allocation: grad_views() maps an extent of it."""

    def __init__(self, params, error=RuntimeError):
        self.params, self.error = list(params), error
        self.offsets = [0]
        for p in self.params:
            self.offsets.append(self.offsets[-1] + (p.numel() + ALIGN - 1) // ALIGN * ALIGN)
        self.n = self.offsets[-1]
        self._off = {id(p): o for p, o in zip(self.params, self.offsets)}
        dev = self.params[0].device
        self.p, self.m, self.v = (torch.zeros(self.n, device=dev, dtype=torch.float32) for _ in range(3))
        self.e = None
        with torch.no_grad():
            for p in self.params:
                view = self.slot(self.p, p)
                view.copy_(p)
                p.data = view

    def slot(self, flat, p):
        """Parameter p's extent of `flat` (p, m, v, e or any tensor laid out like them), in p's shape."""
        off = self._off[id(p)]
        return flat[off:off + p.numel()].view(p.shape)

    def grad_views(self, g):
        """id(parameter) -> its extent of the gradient tensor g (n floats of the owner's allocation)."""
        return {id(p): self.slot(g, p) for p in self.params}

    def start_average(self):
        self.e = self.p.clone()         # (the pads stay zero)

    def tensors(self):
        """Every tensor that is this bucket's state: what a snapshot, a rewind or a broadcast has to cover."""
        return [self.p, self.m, self.v] + ([self.e] if self.e is not None else [])

    def exchange_average(self):
        with torch.no_grad():
            t = self.p.clone()
            self.p.copy_(self.e)
            self.e.copy_(t)

    def decay_mask(self, selected):
        """Which granules of the bucket weight decay covers: a uint8 tensor of n / ALIGN granules on the
        bucket's device, 1 over the granules of the parameters in `selected` (parameters of this bucket, or their ids) and
        0 over the others'.  Every parameter starts at a multiple of ALIGN, so a granule belongs to exactly one
        parameter; the pad behind a parameter's last element lies in that parameter's last granule and stays zero under
        either form of decay (0 * f = 0; 0 + wd * 0 = 0)."""
        chosen = {p if isinstance(p, int) else id(p) for p in selected}
        if chosen - set(self._off):
            raise self.error("decay_mask: %d selected parameter(s) do not live in this bucket" % len(chosen - set(self._off)))
        mask = torch.zeros(self.n // ALIGN, dtype=torch.uint8, device=self.p.device)
        for p, lo, hi in zip(self.params, self.offsets, self.offsets[1:]):
            if id(p) in chosen:
                mask[lo // ALIGN:hi // ALIGN] = 1
        return mask

    def resident(self):
        """Do the parameters still live here?  Only the first and the last are looked at (module.to() / .cuda() move every
        parameter): this runs once per training step, whose host path must not loop over the parameters."""
        base = self.p.data_ptr()
        return self.params[0].data_ptr() == base and self.params[-1].data_ptr() == base + 4 * self.offsets[-2]

    def adam_state(self, order, step, lr, betas, eps, decay=None, decoupled=True):
        """The moments as torch.optim.Adam(order).state_dict() reports them after `step` steps.  Tensors are copies.
        decay: None, or one weight-decay value per parameter of `order` -- the dict is then torch.optim.AdamW's
        (decoupled) or torch.optim.Adam's over ONE PARAM GROUP PER PARAMETER, ids 0..n-1 in the same order, each with its
        own weight_decay (load_adam_state flattens the groups in order, so both layouts load)."""
        state = {}
        if step > 0:
            for i, p in enumerate(order):
                state[i] = {"step": torch.tensor(float(step)), "exp_avg": self.slot(self.m, p).clone(),
                            "exp_avg_sq": self.slot(self.v, p).clone()}
        group = {"lr": lr, "betas": tuple(betas), "eps": eps, "weight_decay": 0, "amsgrad": False, "maximize": False,
                 "foreach": None, "capturable": False, "differentiable": False, "fused": None,
                 "decoupled_weight_decay": False, "params": list(range(len(order)))}
        if decay is None:
            return {"state": state, "param_groups": [group]}
        decay = [float(wd) for wd in decay]
        if len(decay) != len(order):
            raise self.error("adam_state: %d decay values for %d parameters" % (len(decay), len(order)))
        groups = [dict(group, weight_decay=wd, decoupled_weight_decay=bool(decoupled), params=[i])
                  for i, wd in enumerate(decay)]
        return {"state": state, "param_groups": groups}

    def load_adam_state(self, sd, order, what, owner):
        """Fill the moments from a torch.optim.Adam-layout state dict over `order` (a parameter without state gets zeros)
        -> (the set of step counts seen, the first param group).  Nothing is written when the state does not fit.
        what / owner: how the messages name the state and what it was expected to cover."""
        groups = sd["param_groups"]
        ids = [i for g in groups for i in g["params"]]
        if len(ids) != len(order):
            raise self.error("%s holds %d parameters, %s" % (what, len(ids), owner))
        found = []
        for p, i in zip(order, ids):
            st = sd["state"].get(i)
            if not st:
                continue
            if tuple(st["exp_avg"].shape) != tuple(p.shape):
                raise self.error("%s %d has shape %s, parameter has %s" % (what, i, tuple(st["exp_avg"].shape), tuple(p.shape)))
            found.append((p, st))
        with torch.no_grad():
            self.m.zero_()
            self.v.zero_()
            for p, st in found:
                self.slot(self.m, p).copy_(st["exp_avg"])
                self.slot(self.v, p).copy_(st["exp_avg_sq"])
        return {int(float(st["step"])) for _, st in found}, groups[0]
