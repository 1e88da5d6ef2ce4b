"""Case table of the model geometries the suite runs the whole model at (tests/test_model_geometry_cpu.py,
tests/test_model_geometry_gpu.py), and the oracle steps both files compare with.

The geometry decides which Python path a model takes.  With d = emb_dim, ff = the widest feed-forward of the decoder and
entity stacks and NL decoder layers:
  chain      forward row chains            ick_rowchain_supported(ff, d, max(3 d, ff)):  ff <= 512, d <= 320, N2 <= 1024
  chain_bwd  backward row chains           chain and ick_rowchain_bwd_supported(max(3, 2 NL) d, d, ff):  K0 <= 1920
  decode     fused decode kernels          ick_decode_supported: d % 4 == 0, 64 <= d <= 320, H <= 16, d / H <= 32,
                                           decoder_dim % 4 == 0, decoder_dim <= 1024 (16 chunks of 64), S <= 1024
  derived    TrainStep's DerivedWeights    chain_bwd, every weight's row length a multiple of 4 floats (d % 4 == 0) and
                                           V % 8 == 0: fc_vocab's transposed bf16 planes are written 8 rows at a time
                                           (weights.py: DerivedWeights._tables)
so the tiers are: full (chains both ways and the fused decode), mixed (forward chains, unfused backward, staged per-step
packing), chains off with the fused decode still on, and everything off.  The columns below are derived by hand from
those constants; the CPU test holds chain / chain_bwd / decode to the library's predicates, the GPU test holds every
column to what the model does.

Every case: B = 5 captions of L = 9 positions, K = 6 entities, seed 21 (caption lengths 5, 6, 9, 7, 8).  CASES, the twelve
geometries, have V = 150 words: 150 % 8 = 6, so NONE of them gets DerivedWeights, whatever its geometry -- their re-laid-
out weight images are re-packed by per-step launches (staged in the mixed tier).  DERIVED_CASES repeat the six geometries
that admit DerivedWeights at V = 152, where the Adam pass writes the images itself; they run the tier, train-step and
three-step checks (the decode and eval-forward paths do not depend on the vocabulary's alignment).
"""
import contextlib
from dataclasses import dataclass, replace

import torch

import ick_amd.synth as synth
from decode_ref import float64_default, params64
from oracle import restatement as R

B, L, K, V, SEED = 5, 9, 6, 150, 21
LENGTHS = [5, 6, 9, 7, 8]
MAX_LEN = 9                      # greedy / beam decode length of the decode checks
LR, CLIP = 4e-4, 5.0
STEP_SEEDS = (21, 22, 21)        # the batches of the three-step sequence

# the limits the table is built around (csrc/rowchain.h, csrc/rowchain_bwd.hip, csrc/decode.hip, ops.DHP)
MAX_K, MAX_D, MAX_N2, MAX_K0, MAX_HEAD = 512, 320, 1024, 1920, 32


@dataclass(frozen=True)
class Case:
    name: str
    variant: str
    d: int
    H: int
    FF_dec: int
    FF_enc: int
    NL: int
    P: int
    Fn: int
    chain: bool
    chain_bwd: bool
    decode: bool
    derived: bool
    why: str = ""
    V: int = 150

    @property
    def ff(self):
        return max(self.FF_dec, self.FF_enc)

    @property
    def K0(self):
        """Columns the widest backward pre-GEMM is handed: in_proj's 3 d, or the all-layer cross K/V gradient's 2 NL d."""
        return max(3, 2 * self.NL) * self.d

    @property
    def tier(self):
        if self.chain and self.chain_bwd and self.decode:
            return "full"
        if self.chain and not self.chain_bwd:
            return "mixed"
        if not self.chain and self.decode:
            return "no_chains"
        if not self.chain and not self.decode:
            return "none"
        return "partial"

    @property
    def S(self):
        return self.P + K + self.Fn

    @property
    def geometry(self):
        """The keyword arguments tests/test_bench_sizes_gpu.py's helpers take."""
        return dict(d=self.d, H=self.H, decoder_dim=self.FF_dec, encoder_dim=self.FF_enc, num_layers=self.NL, P=self.P)


def _c(name, variant, geo, chain, chain_bwd, decode, why):
    d, H, FF_dec, FF_enc, NL, P, Fn = geo
    return Case(name, variant, d, H, FF_dec, FF_enc, NL, P, Fn, chain, chain_bwd, decode, False, why)


Y, N = True, False
CASES = [
    _c("base", "geo", (300, 10, 512, 512, 3, 196, 0), Y, Y, Y, "the geometry every other test runs at"),
    _c("deep_geo", "geo", (300, 10, 512, 512, 4, 196, 0), Y, N, Y, "K0 = 2400 > 1920: forward chains, unfused backward"),
    _c("deep_knowledge", "knowledge", (300, 10, 512, 512, 4, 196, 5), Y, N, Y, "mixed tier with the fact stack"),
    _c("single_layer", "knowledge", (300, 10, 512, 512, 1, 196, 5), Y, Y, Y,
       "nseg = 2 < 3: K0 = 3 d = 900, no layer receives a handed-over q|k|v"),
    _c("limit_geo", "geo", (320, 10, 512, 512, 3, 49, 0), Y, Y, Y,
       "d = 320, N2 = 960, K0 = 1920 exactly, head width 32: no pad columns"),
    _c("limit_knowledge", "knowledge", (320, 10, 512, 512, 3, 49, 5), Y, Y, Y, "the same limits with facts"),
    _c("wide_ffn", "knowledge", (300, 10, 1024, 512, 2, 196, 5), N, N, Y,
       "decoder_dim 1024 > 512: no chains; 16 chunks = kPartsMax in the fused decode"),
    _c("wide_ctx", "geo", (300, 10, 512, 768, 3, 196, 0), N, N, Y, "the entity stack's 768 turns the chains off"),
    _c("wide_model", "geo", (384, 12, 384, 384, 2, 196, 0), N, N, N, "d = 384 > 320: per-op launches everywhere"),
    _c("news_small", "news", (256, 8, 384, 320, 2, 196, 5), Y, Y, Y, "news through the captured step"),
    _c("odd_head", "geo", (152, 8, 256, 256, 2, 196, 0), Y, Y, Y, "head width 19"),
    _c("unaligned", "geo", (150, 10, 256, 256, 2, 196, 0), Y, Y, N,
       "d % 4 = 2, head width 15: chains packed from unaligned rows, no fused decode, no DerivedWeights"),
]
V_ALIGNED = 152
DERIVED_CASES = [replace(c, name=c.name + "_v152", V=V_ALIGNED, derived=True,
                         why=c.why + "; V = 152: the Adam pass writes the weight images")
                 for c in CASES if c.chain_bwd and c.d % 4 == 0]
ALL_CASES = CASES + DERIVED_CASES
BY_NAME = {c.name: c for c in ALL_CASES}
assert len(BY_NAME) == len(ALL_CASES)

# (variant, d, H, FF_dec, FF_enc, NL): head width 64 > 32, which the head-major buffers (ops.DHP floats per head) cannot hold
REFUSED = [("geo", 320, 5, 512, 512, 2)]

# beam search against the CPU beam reference runs on these (fused decode on; one seed)
BEAM_CASES = ["deep_knowledge", "limit_knowledge", "wide_ffn", "odd_head"]


# ------------------------------------------------------------------------------------------------ inputs and models
def make_params(c):
    return synth.make_params(c.variant, c.V, SEED, d=c.d, decoder_dim=c.FF_dec, encoder_dim=c.FF_enc, num_layers=c.NL)


def make_inputs(c, seed=SEED):
    """(batch, enc_out) of one step."""
    return synth.make_batch(c.variant, B, L, K, c.V, c.Fn, seed), synth.make_enc_out(B, seed, emb_dim=c.d, P=c.P)


def oracle_config(c):
    return R.config_from_word_map(c.variant, synth.make_word_map(c.V), emb_dim=c.d, num_heads=c.H, num_layers=c.NL)


def build_model(variant, d, H, FF_dec, FF_enc, NL, P=None, V=V):
    """The drop-in module on the GPU in eval mode, as tests/test_decode_gpu.py::test_fused_decode_other_model_sizes
    builds it.  P: the parameters to load (None keeps the constructor's)."""
    import ick_amd
    m = ick_amd.load_models(variant)
    dec = m.DecoderTransformer(word_map=synth.make_word_map(V), emb_dim=d, decoder_dim=FF_dec, encoder_dim=FF_enc,
                               num_heads=H, num_layers=NL)
    if P is not None:
        missing, unexpected = dec.load_state_dict(P, strict=False)
        assert missing == ["pos_encoder.pe"] and not unexpected
    return dec.cuda().eval()


def build_decoder(c, P):
    return build_model(c.variant, c.d, c.H, c.FF_dec, c.FF_enc, c.NL, P, c.V)


def step_args(batch, enc_out):
    args = [batch["captions"].cuda(), enc_out.cuda(), batch["caption_masks"].cuda(), batch["caption_lengths"].cuda(),
            batch["entities"]]
    if "facts" in batch:
        args.append(batch["facts"].cuda())
    return args


# ------------------------------------------------------------------------------------------------ the oracle
def _trainable(P, f64):
    src = params64(P) if f64 else P
    Pr = {k: v.clone().requires_grad_(True) for k, v in src.items() if not k.startswith("fact_encoder.")}
    if "predicate_embedding.weight" in Pr:
        Pr["fact_encoder.predicate_embedding.weight"] = Pr["predicate_embedding.weight"]
    return Pr


def _forward_loss(cfg, Pr, batch, enc_out, f64):
    scores, caps, dl = R.forward(cfg, Pr, batch["captions"], enc_out.double() if f64 else enc_out, batch["caption_masks"],
                                 batch["caption_lengths"], batch["entities"], batch.get("facts"))
    return scores, caps, dl, R.packed_ce_loss(cfg, scores, caps, dl)


def oracle_step(c, f64, P=None, inputs=None):
    """One oracle step of case c -- R.forward, R.packed_ce_loss, backward -- in float32, as
    tests/test_bench_sizes_gpu.py::reference_train_step runs it, or in float64.  inputs: a (batch, enc_out) in place of
    the case's own (tests/batch_cases.py).  -> dict(loss, scores (B, L, Vx) in length order, valid (B, L) bool, grads by
    name)."""
    P = make_params(c) if P is None else P
    cfg = oracle_config(c)
    batch, enc_out = make_inputs(c) if inputs is None else inputs
    with (float64_default() if f64 else contextlib.nullcontext()):
        Pr = _trainable(P, f64)
        scores, caps, dl, loss = _forward_loss(cfg, Pr, batch, enc_out, f64)
        loss.backward()
    valid = torch.arange(scores.shape[1]).view(1, -1) < torch.tensor(dl).view(-1, 1)
    grads = {k: (v.grad if v.grad is not None else torch.zeros_like(v)).detach()
             for k, v in Pr.items() if not k.startswith("fact_encoder.")}
    return dict(loss=loss.item(), scores=scores.detach(), valid=valid, grads=grads, decode_lengths=dl)


def oracle_loss_sequence(c, P=None, inputs=None, f64=True):
    """The float64 oracle's losses over STEP_SEEDS' batches with torch Adam (lr 4e-4) on gradients clamped to +-5.
    inputs: a list of (batch, enc_out), of any shapes, in place of those batches; f64=False: the same sequence in float32
    (the reference's own noise over a sequence, tests/test_batch_geometry_cpu.py)."""
    P = make_params(c) if P is None else P
    cfg = oracle_config(c)
    losses = []
    if inputs is None:
        inputs = [make_inputs(c, seed) for seed in STEP_SEEDS]  # (drawn in float32: synth draws with the default dtype)
    with (float64_default() if f64 else contextlib.nullcontext()):
        Pr = _trainable(P, f64)
        uniq = [v for k, v in Pr.items() if not k.startswith("fact_encoder.")]
        opt = torch.optim.Adam(uniq, lr=LR)
        for batch, enc_out in inputs:
            opt.zero_grad()
            loss = _forward_loss(cfg, Pr, batch, enc_out, f64)[3]
            loss.backward()
            for p in uniq:
                if p.grad is not None:
                    p.grad.clamp_(-CLIP, CLIP)
            opt.step()
            losses.append(loss.item())
    return losses
