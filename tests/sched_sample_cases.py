"""The step-level cases of the scheduled-sampling tests (tests/test_sched_sample_cpu.py, tests/test_sched_sample_gpu.py)
and their float64 oracle: tests/model_cases.py's `base` (geo) and `single_layer` (knowledge) geometries at B = 5, L = 9,
K = 6, V = 152 (the aligned vocabulary: the Adam pass writes the weight images), seed 21, prob = 1 in argmax mode.

The oracle: R.forward on the gold captions gives the teacher-forced scores; at every eligible position (b, q),
1 <= q <= lengths[b] - 2, the fed token becomes the lowest column holding the maximum of the scores of position q - 1,
<start> and <pad> excluded, with the mask of its column range; R.forward on those mixed inputs, the packed cross entropy
against the GOLD captions, backward."""
import torch

import model_cases as MC
from decode_ref import float64_default
from oracle import restatement as R

CASES = [MC.BY_NAME["base_v152"], MC.BY_NAME["single_layer_v152"]]
# The parameters are seed 21's (model_cases.SEED); the INPUTS are seed 25's: at seed 21 the float64 oracle's smallest
# top-two margin over the eligible positions is 1.5e-4 (base) / 4.2e-4 (single_layer), below the 1e-3 the GPU test's
# exact comparison of the mixed inputs needs (test_sched_sample_cpu.py::test_oracle_margin_precondition); at seed 25 it
# is 1.2e-2 / 4.3e-3, with 10 pointer tokens fed back in the knowledge case.
SEED = 25
STEP_SEEDS = (25, 26, 25)
MIN_MARGIN = 1e-3
_CACHE = {}


def mixed_inputs(c, scores, sort_ind, batch):
    """scores: float64 teacher-forced scores in length order -> (captions_in, masks_in, replaced, margins) in the batch's
    own order; margins: the top-two margin, banned columns excluded, of every eligible position."""
    wm = MC.synth.make_word_map(c.V)
    caps, masks = batch["captions"].clone(), batch["caption_masks"].clone()
    replaced = torch.zeros_like(caps, dtype=torch.int32)
    lengths = batch["caption_lengths"].view(-1).tolist()
    margins = {}
    for r, b in enumerate(sort_ind.tolist()):
        for q in range(1, min(lengths[b] - 1, MC.L - 1)):
            s = scores[r, q - 1].clone()
            s[wm["<start>"]] = s[wm["<pad>"]] = float("-inf")
            top = s.topk(2)
            col = int((s == top.values[0]).nonzero()[0])
            margins[(b, q)] = float(top.values[0] - top.values[1])
            caps[b, q], masks[b, q], replaced[b, q] = col, 0 if col < c.V else (1 if col < c.V + MC.K else 2), 1
    return caps, masks, replaced, margins


def oracle(c, seed=SEED):
    """dict(P, batch, enc_out, captions_in, masks_in, replaced, margins, loss, grads) of the case's first step."""
    key = (c.name, seed)
    if key in _CACHE:
        return _CACHE[key]
    P = MC.make_params(c)
    cfg = MC.oracle_config(c)
    batch, enc_out = MC.make_inputs(c, seed)
    with float64_default():
        Pr = MC._trainable(P, True)
        with torch.no_grad():
            stages = {}
            scores, _, _ = R.forward(cfg, Pr, batch["captions"], enc_out.double(), batch["caption_masks"],
                                     batch["caption_lengths"], batch["entities"], batch.get("facts"), stages=stages)
        sort_ind = stages["sort_ind"]
        caps_in, masks_in, replaced, margins = mixed_inputs(c, scores, sort_ind, batch)
        scores2, _, dl = R.forward(cfg, Pr, caps_in, enc_out.double(), masks_in, batch["caption_lengths"],
                                   batch["entities"], batch.get("facts"))
        loss = R.packed_ce_loss(cfg, scores2, batch["captions"][sort_ind], dl)      # the targets stay gold
        loss.backward()
    grads = {k: (v.grad if v.grad is not None else torch.zeros_like(v)).detach()
             for k, v in Pr.items() if not k.startswith("fact_encoder.")}
    out = dict(P=P, batch=batch, enc_out=enc_out, captions_in=caps_in, masks_in=masks_in, replaced=replaced,
               margins=margins, loss=loss.item(), grads=grads)
    _CACHE[key] = out
    return out


# ------------------------------------------------------------------------------------------------ the kernel alone
# (name, V, K, F, B, L, lengths): Vx = 52 (a multiple of 4), 161, 10 026, 50 071; B * L from 2 to 130 rows; L = 2; every
# length 1 (no packed row at all); every length 2 (rows, none eligible)
KERNEL_SHAPES = [
    ("v52", 40, 7, 5, 3, 7, [7, 4, 9]),
    ("v161", 150, 6, 5, 5, 9, [5, 6, 9, 7, 8]),
    ("v10026", 10000, 20, 6, 4, 6, [6, 3, 5, 6]),
    ("v50071", 50000, 20, 51, 2, 5, [5, 4]),
    ("rows130", 150, 6, 0, 13, 10, [10, 3, 7, 1, 12, 5, 2, 9, 10, 4, 8, 6, 10]),
    ("rows2", 150, 6, 0, 1, 2, [2]),
    ("L2", 150, 6, 5, 3, 2, [1, 2, 5]),
    ("all_length_1", 150, 6, 5, 3, 5, [1, 1, 1]),
    ("all_length_2", 150, 6, 5, 3, 5, [2, 2, 2]),
]
LAYOUTS = ("tight", "padded", "offset")
KERNEL_SEED, KERNEL_STEP = 0x5EED0123456789, 3


def kernel_case(name):
    """-> dict of one kernel-alone case: packed score rows of exact eighths (M', Vx) float32, gold captions / masks,
    lengths and the token ids, from a generator seeded by the name."""
    _, V, K, F, B, L, lengths = next(s for s in KERNEL_SHAPES if s[0] == name)
    Vx = V + K + F
    gen = torch.Generator().manual_seed(sum(map(ord, name)))
    M = sum(min(L - 1, max(0, n - 1)) for n in lengths)
    rows = torch.randint(-32, 33, (M, Vx), generator=gen).float() / 8
    caps = torch.randint(1, Vx, (B, L), generator=gen)
    start, pad = V - 2, 0
    caps[:, 0] = start
    for b, n in enumerate(lengths):
        caps[b, min(n, L):] = pad
    masks = (caps >= V).long() + (caps >= V + K).long()
    if M > 0:                         # banned columns that hold the maximum must lose, in every row
        rows[:, start] = 5.0
        rows[:, pad] = 5.0
    return dict(name=name, V=V, K=K, F=F, B=B, L=L, Vx=Vx, lengths=lengths, rows=rows, captions=caps, masks=masks,
                start=start, pad=pad, M=M)
