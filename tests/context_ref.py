"""Plain float64 references of the context, embedding and pointer kernels (csrc/prefill.hip, the scatter kernels of
csrc/backward.hip, pointer_scores_kernel of csrc/score_head.hip), written against the kernels' documented contract:
out-of-range indices clamp (deviation 2) except in the context indicators, where a fact whose subject or
predicate is out of range is simply not active.  Nothing here imports the package under test.

Every function is differentiable in its float operands, so the backward references are torch.autograd on them
(`grads`).  Every function also has an `*_abs` evaluation: the same computation with every float operand (and, in
`grads(..., absval=True)`, the upstream gradient) replaced by its absolute value, which gives per output element the sum
of the absolute values of its addends -- the A of the tolerance (n + 4) * 2^-24 * A (`bound`).
"""
import torch

TYPE_OFFSET = {"geo": 4, "knowledge": 6, "news": 5}
U = 2.0 ** -24          # unit roundoff of float32


def _d(x):
    return x if x.dtype == torch.float64 else x.double()


def A(x, absval):
    """A float operand as float64, or its absolute value for an `*_abs` evaluation."""
    return _d(x).abs() if absval else _d(x)


# ------------------------------------------------------------------------------------------ EntityEncoder.forward
def fact_counts(facts, K):
    """(B, K) number of facts whose subject is the entity; 0 for the last row (<unk_ent>).  Compared as int64: a subject
    such as 2^32 + 1 matches no entity."""
    B, F, _ = facts.shape
    out = torch.zeros(B, K, dtype=torch.float64)
    for b in range(B):
        for j in range(F):
            s = int(facts[b, j, 1])
            if 0 <= s < K - 1:
                out[b, s] += 1.0
    return out


def clamp_type(entities, ntypes):
    """Type index: the float truncated toward zero, then clamped to [0, ntypes - 1]."""
    return entities[:, :, 4].double().trunc().clamp(0, ntypes - 1).long()


def clamp_names(entities, vocab):
    return entities[:, :, 5:10].double().trunc().clamp(0, vocab - 1).long()


def entity_encode(variant, entities, type_emb, d, facts=None, word_emb=None, absval=False):
    """entities (B, K, cols) float32, type_emb (ntypes, d - type_offset), word_emb (vocab, d) for news -> (B, K, d)."""
    ent = _d(entities)
    B, K, _ = ent.shape
    off = TYPE_OFFSET[variant]
    assert type_emb.shape[1] == d - off
    slots = torch.zeros(B, K, off, dtype=torch.float64)
    count = fact_counts(facts, K) if variant != "geo" else None
    if variant == "news":
        slots[:, :, 0], slots[:, :, 1], slots[:, :, 2] = ent[:, :, 1], ent[:, :, 2], ent[:, :, 3]
        slots[:, :, 3], slots[:, :, 4] = count, (count > 0).double()
    else:
        az = ent[:, :, 2]                       # get_dist_to_north / get_dist_to_east in double, like the reference
        slots[:, :, 0] = ent[:, :, 1]
        slots[:, :, 1] = az.abs() / 180.0
        slots[:, :, 2] = torch.where(az >= -90.0, (90.0 - az).abs(), 90.0 + (az + 180.0).abs()) / 180.0
        slots[:, :, 3] = ent[:, :, 3]
        if variant == "knowledge":
            slots[:, :, 4], slots[:, :, 5] = count, (count > 0).double()
    if absval:
        slots = slots.abs()
    enc = torch.cat([slots, _d(type_emb)[clamp_type(entities, type_emb.shape[0])]], dim=2)
    if variant == "news":
        rows = _d(word_emb)[clamp_names(entities, word_emb.shape[0])]     # (B, K, 5, d)
        s = rows[:, :, 0]
        for w in range(1, 5):                   # sum in order, then divide
            s = s + rows[:, :, w]
        enc = enc * (s / 5.0)
    return enc


def entity_encode_abs(variant, entities, type_emb, d, facts=None, word_emb=None):
    words = None if word_emb is None else _d(word_emb).abs()
    return entity_encode(variant, entities, _d(type_emb).abs(), d, facts, words, absval=True)


# -------------------------------------------------------------------------------------------- FactEncoder.forward
def clamp_facts(facts, K, num_pred):
    """(subject, predicate) rows clamped in int64 to [0, K - 1] / [0, num_pred - 1]."""
    return facts[:, :, 1].clamp(0, K - 1), facts[:, :, 2].clamp(0, num_pred - 1)


def fact_encode(facts, ee, pred_emb, absval=False):
    ee, pred_emb = _d(ee), _d(pred_emb)
    B, K, d = ee.shape
    subj, pred = clamp_facts(facts, K, pred_emb.shape[0])
    return torch.gather(ee, 1, subj.unsqueeze(2).expand(-1, -1, d)) + pred_emb[pred]


def fact_encode_abs(facts, ee, pred_emb):
    return fact_encode(facts, _d(ee).abs(), _d(pred_emb).abs())


# ---------------------------------------------------------------------------------------- CaptionEmbedder.forward
def caption_sources(captions, masks, V, K, F, pad, has_facts):
    """Per caption position the table it reads ("word" / "ent" / "fact") and the row: mask 1 -> entity row (a pointer
    outside [V, V + K) -> K - 1), mask 2 with facts -> fact row (outside -> F - 1), anything else -> word row (a token
    >= V or < 0 -> <pad>).  Entity / fact rows are per sample."""
    B, L = captions.shape
    kind = [[None] * L for _ in range(B)]
    row = torch.zeros(B, L, dtype=torch.long)
    for b in range(B):
        for l in range(L):
            tok, m = int(captions[b, l]), int(masks[b, l])
            if m == 1:
                e = tok - V
                kind[b][l], row[b, l] = "ent", (e if 0 <= e < K else K - 1)
            elif m == 2 and has_facts:
                f = tok - V - K
                kind[b][l], row[b, l] = "fact", (f if 0 <= f < F else F - 1)
            else:
                kind[b][l], row[b, l] = "word", (tok if 0 <= tok < V else pad)
    return kind, row


def caption_embed(captions, masks, word_emb, ee, fe, pe, V, pad, scale, pos0=0, mask=None, round32=False, absval=False):
    """-> (x, emb): emb the gathered rows, x = (emb * scale + pe[pos0 + l]) * mask.  `scale` is the float32 the kernel
    receives.  round32: the product is rounded to float32 before the sum and the sum before the mask, as the kernel
    documents (a multiply, an add, a multiply -- no fused operation), so that x rounded to float32 is the kernel's
    result bit for bit; without it the arithmetic is plain float64 (the form that is differentiated)."""
    word_emb, ee, pe = _d(word_emb), _d(ee), _d(pe)
    fe = None if fe is None else _d(fe)
    B, L = captions.shape
    K, d = ee.shape[1], ee.shape[2]
    F = 0 if fe is None else fe.shape[1]
    kind, row = caption_sources(captions, masks, V, K, F, pad, fe is not None)
    rows = []
    for b in range(B):
        for l in range(L):
            r, k = int(row[b, l]), kind[b][l]
            rows.append(word_emb[r] if k == "word" else (ee[b, r] if k == "ent" else fe[b, r]))
    emb = torch.stack(rows).view(B, L, d)
    sc = torch.tensor(float(scale), dtype=torch.float32).double()
    per = pe[pos0:pos0 + L].unsqueeze(0)
    if absval:
        sc, per = sc.abs(), per.abs()
    x = emb * sc
    if round32:
        x = x.float().double()
    x = x + per
    if mask is not None:
        if round32:
            x = x.float().double()
        x = x * (_d(mask).abs() if absval else _d(mask)).view(B, L, d)
    return x, emb


def caption_embed_abs(captions, masks, word_emb, ee, fe, pe, V, pad, scale, pos0=0, mask=None):
    return caption_embed(captions, masks, _d(word_emb).abs(), _d(ee).abs(), None if fe is None else _d(fe).abs(), pe, V,
                         pad, scale, pos0, mask, absval=True)


# ----------------------------------------------------------------------------------------- get_context_indicators
def indicator_tables(captions, facts, K, V, num_pred, mode):
    """-> eib (B, T, F), dense predicate indicator (B, T, num_pred), both 0/1 float64.  T = L in mode 0 (position p sees
    the entity pointers at positions < p) and 1 in mode 1 (one row that sees every pointer of the caption).  A fact whose
    subject is outside [0, K) is never active; one whose predicate is outside [0, num_pred) marks no predicate."""
    B, L = captions.shape
    F = facts.shape[1]
    T = L if mode == 0 else 1
    eib = torch.zeros(B, T, F, dtype=torch.float64)
    pi = torch.zeros(B, T, max(num_pred, 1), dtype=torch.float64)
    for b in range(B):
        first = {}
        for t in range(L):
            n = int(captions[b, t]) - V
            if 0 <= n < K and n not in first:
                first[n] = t
        for j in range(F):
            s, q = int(facts[b, j, 1]), int(facts[b, j, 2])
            if not (0 <= s < K and s in first):
                continue
            act = first[s] + 1 if mode == 0 else 0
            for p in range(act, T):
                eib[b, p, j] = 1.0
                if 0 <= q < num_pred:
                    pi[b, p, q] = 1.0
    return eib, pi[:, :, :num_pred]


def context_indicators(captions, facts, K, V, weight, bias, mode=0, absval=False):
    """weight (d, num_pred) and bias (d,) of fc_predicate -> (eib, gate (B, T, d), dense predicate indicator)."""
    weight, bias = _d(weight), _d(bias)
    eib, pi = indicator_tables(captions, facts, K, V, weight.shape[1], mode)
    return eib, pi @ weight.t() + bias, pi


def context_indicators_abs(captions, facts, K, V, weight, bias, mode=0):
    return context_indicators(captions, facts, K, V, _d(weight).abs(), _d(bias).abs(), mode)


# ------------------------------------------------------------------------------------- pointer part of get_scores
def pointer_scores(h, ctx, w, bias, ind=None, absval=False):
    """h (B, T, d), ctx (B, Kc, d), w (1, d), bias (1,), ind (B, T, Kc) or None -> ind * sum_d h ctx w + bias."""
    h, ctx, w, bias = _d(h), _d(ctx), _d(w), _d(bias)
    s = ((h.unsqueeze(2) * ctx.unsqueeze(1)) * w.view(1, 1, 1, -1)).sum(-1)
    if ind is not None:
        s = s * (_d(ind).abs() if absval else _d(ind))
    return s + bias.view(1, 1, 1)


def pointer_scores_abs(h, ctx, w, bias, ind=None):
    return pointer_scores(_d(h).abs(), _d(ctx).abs(), _d(w).abs(), _d(bias).abs(), ind, absval=True)


# ------------------------------------------------------------------------------------------------------ backward
def grads(fn, leaves, upstream, absval=False):
    """torch.autograd through `fn(**leaf tensors)` in float64: -> {name: gradient}.  `leaves` maps the names of the float
    operands to differentiate to their values; `fn` closes over everything else, takes `absval` and passes the float
    operands it closes over through A(x, absval).  absval: leaves and upstream gradient are replaced by their absolute
    values as well, giving the sum of |addends| of every gradient element."""
    lv = {k: (_d(v).abs() if absval else _d(v)).clone().requires_grad_(True) for k, v in leaves.items()}
    out = fn(absval=absval, **lv)
    up = _d(upstream).abs() if absval else _d(upstream)
    got = torch.autograd.grad(out, list(lv.values()), up, allow_unused=True)
    return {k: (torch.zeros_like(v) if g is None else g) for (k, v), g in zip(lv.items(), got)}


def bound(n, A):
    """Elementwise |got - ref| allowed for a float32 sum of n addends whose absolute values sum to A: any summation order
    errs by at most (n - 1) u A to first order, and the +4 covers the roundings inside one addend (a product of up to
    four factors)."""
    return (n + 4) * U * A
