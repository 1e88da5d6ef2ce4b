"""ick_decode_layers_attn without a device: declared in the C header, exported by the library, bound in lib.py with
the argument types of ick_decode_layers_part plus the weight buffer; the argument errors the host can see are raised."""
import os
import re
import subprocess

import pytest

import ick_amd.decoder as D
import ick_amd.lib as L
import ick_amd.ops as ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "ick_amd.h")).read()
    assert re.search(r"int ick_decode_layers_attn\(const ick_decode_ctx\* ctx, float\* attn, int32_t pos, int32_t part, "
                     r"void\* stream\);", hdr)
    assert L.SIGNATURES["ick_decode_layers_attn"] == [L.SIGNATURES["ick_decode_layers_part"][0], L.C.c_void_p] + \
        L.SIGNATURES["ick_decode_layers_part"][1:]
    lib = L.load()
    assert lib.ick_decode_layers_attn.argtypes == L.SIGNATURES["ick_decode_layers_attn"]
    syms = subprocess.run(["nm", "-D", "--defined-only", L.load()._name], capture_output=True, text=True).stdout
    assert re.search(r"\bT ick_decode_layers_attn\b", syms)


def test_host_side_argument_errors():
    ctx = L.DecodeCtx()
    ctx.R, ctx.layers, ctx.H, ctx.S, ctx.max_len = 2, 1, 2, 8, 4
    # a bad part or a null context fails in the library before anything is launched
    with pytest.raises(L.IckError):
        ops.decode_layers_attn(ctx, None, 0, 3)
    assert L.load().ick_decode_layers_attn(None, None, 0, 0, None) != 0
    assert L.load().ick_decode_layers_attn(ctx, None, 0, 5, None) != 0
    # the context has no buffers: the argument checks refuse it with or without a weight buffer
    assert L.load().ick_decode_layers_attn(ctx, None, 0, 0, None) != 0
    import torch
    with pytest.raises(L.IckError):                       # not a device tensor
        ops.decode_layers_attn(ctx, torch.zeros(4, 2, 1, 2, 8), 0)


def test_attention_buffer_limit_and_split():
    import torch
    D._attention_check("predict", 20, 32, 3, 10, 216)    # cfg5 greedy: 16.6 MB
    with pytest.raises(L.IckError):
        D._attention_check("predict", 128, 65535, 3, 16, 1024)
    w = torch.rand(3, 2, 196 + 5 + 4)
    parts = D.split_attention(w, 196, 5, 4)
    assert parts["image"].shape == (3, 2, 14, 14) and parts["entities"].shape == (3, 2, 5)
    assert parts["facts"].shape == (3, 2, 4)
    assert torch.equal(parts["image"][1, 0, 2, 3], w[1, 0, 2 * 14 + 3])
    assert torch.equal(parts["facts"], w[..., 201:])
    assert D.split_attention(torch.rand(2, 10 + 3), 10, 3)["image"].shape == (2, 10)   # not a square grid
    with pytest.raises(L.IckError):
        D.split_attention(w, 196, 5)


def test_zero_after_end():
    import torch
    tok = torch.tensor([[5, 2, 9, 0], [5, 6, 7, 8]])          # <end> = 9
    a = torch.ones(4, 2, 3)
    D._zero_after_end(a, tok, 9)
    assert a[:, 0, 0].tolist() == [1, 1, 1, 0] and a[:, 1, 0].tolist() == [1, 1, 1, 1]
