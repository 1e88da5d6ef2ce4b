"""CPU checks of the device CIDEr-D: the restatement against hand-computed values, the package's host-built df table
against the restatement's, the exported symbol, and argument errors before any launch."""
import ctypes
import math
import os

import numpy as np
import pytest

from cider_ref import cider_d, doc_freq, table_to_dict

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
START, END, PAD = 98, 99, 0
WM = {"<start>": START, "<end>": END, "<pad>": PAD}


@pytest.fixture(scope="module")
def built_lib():
    import ick_amd.build as build
    return build.build()


def _row(ws, L=8):
    r = [START] + list(ws) + [END]
    return r + [PAD] * (L - len(r))


# ------------------------------------------------------------------------------------------------ restatement
def test_restatement_hand_computed_values():
    corpus = [[_row([1, 2, 3])], [_row([4, 5, 6])]]
    df, lrl = doc_freq(corpus, START, END, PAD)
    assert lrl == math.log(2.0) and df[(1, 2, 3)] == 1 and df[(4,)] == 1
    # s1 = s2 = s3 = 1 (identical vectors, equal length), s4 = 0 (no 4-grams): (1 + 1 + 1 + 0) / 4 * 10
    assert abs(cider_d(_row([1, 2, 3]), corpus[0], df, lrl, START, END, PAD) - 7.5) < 1e-12
    assert cider_d(_row([]), corpus[0], df, lrl, START, END, PAD) == 0.0                 # empty candidate
    assert cider_d([END] * 8, corpus[0], df, lrl, START, END, PAD) == 0.0
    # a duplicated reference (M = 2 of the same row) leaves the score unchanged
    for cand in (_row([1, 2, 3]), _row([1, 2, 5, 6]), _row([3, 2, 1, 2])):
        one = cider_d(cand, corpus[0], df, lrl, START, END, PAD)
        two = cider_d(cand, corpus[0] * 2, df, lrl, START, END, PAD)
        assert abs(one - two) < 1e-12


def test_restatement_words_rule():
    from cider_ref import words
    # <pad> and ignored ids close the gap; nothing after <end>; pointer ids (>= V) stay ids
    assert words([START, 1, PAD, 2, 7, 150, END, 3], START, END, PAD, ignore=(7,)) == [1, 2, 150]
    assert words([1, 2, 3], START, END, PAD) == [1, 2, 3]                           # no <end>: every token


# ------------------------------------------------------------------------------------------------ df table
def _random_corpus(seed, N_img=40, M=3, L=14, V=30):
    rng = np.random.default_rng(seed)
    c = rng.integers(1, 12, size=(N_img, M, L)).astype(np.int64)         # a small alphabet: many repeated n-grams
    c[..., 0] = START
    c[rng.random(c.shape) < 0.08] = PAD                                  # <pad> gaps inside captions
    c[rng.random(c.shape) < 0.08] = 5                                    # an ignored id
    c[rng.random(c.shape) < 0.10] = V + rng.integers(0, 6)               # pointer ids
    ends = rng.integers(1, L + 2, size=(N_img, M))                       # L + 1: no <end> at all
    for i in range(N_img):
        for m in range(M):
            if ends[i, m] < L:
                c[i, m, ends[i, m]] = END
                c[i, m, ends[i, m] + 1:] = PAD
    c[3, 1] = c[3, 0]                                                    # an image with two equal references
    c[7, 2] = [END] + [PAD] * (L - 1)                                    # an empty reference
    return c


@pytest.mark.parametrize("ignore", [(), (5, 11)])
def test_df_table_matches_restatement(ignore):
    from ick_amd.cider import df_table
    c = _random_corpus(3)
    keys, counts, lrl = df_table(c, WM, ignore)
    df, lrl_ref = doc_freq([list(img) for img in c], START, END, PAD, ignore)
    assert lrl == lrl_ref
    assert keys.dtype == np.uint32 and keys.shape[1] == 4 and counts.dtype == np.int32
    assert table_to_dict(keys, counts) == df
    # sorted, unique, unused slots 0xFFFFFFFF
    k = [tuple(r) for r in keys.tolist()]
    assert k == sorted(set(k))
    assert max(df.values()) > 1 and any(len(g) == 4 for g in df)         # repeats across images, all n
    # the union counts once per image: image 3's two equal references count once
    assert all(v <= c.shape[0] for v in df.values())
    # a (N_img, L) corpus is one reference per image
    keys1, counts1, _ = df_table(c[:, 0], WM, ignore)
    assert table_to_dict(keys1, counts1) == doc_freq([[r] for r in c[:, 0]], START, END, PAD, ignore)[0]


def test_df_table_rejects_bad_corpora():
    from ick_amd.cider import df_table
    from ick_amd.lib import IckError
    with pytest.raises(IckError):
        df_table(np.array([[START, END, PAD]]), WM)                    # no n-grams
    with pytest.raises(IckError):
        df_table(np.array([[START, 3, -4, END]]), WM)                  # negative id
    with pytest.raises(IckError):
        df_table(np.array([[START, 3, 2 ** 31, END]]), WM)             # id past 2^31 - 2
    with pytest.raises(IckError):
        df_table(np.zeros((2, 2, 2, 2), dtype=np.int64), WM)


# ------------------------------------------------------------------------------------------------ C ABI
def test_header_and_library_export_cider(built_lib):
    with open(os.path.join(ROOT, "include", "ick_amd.h")) as f:
        assert "int ick_cider_d(" in f.read()
    assert hasattr(ctypes.CDLL(built_lib), "ick_cider_d")
    import ick_amd
    from ick_amd.cider import CiderD
    assert ick_amd.CiderD is CiderD


def test_bad_arguments_are_einval_before_any_launch(built_lib):
    import ick_amd.lib as L
    lib = L.load()
    p = ctypes.c_void_p(16)              # never dereferenced: every call below fails its checks before a launch
    ign = (ctypes.c_int32 * 16)()
    ok = dict(cand=p, N=6, T=20, refs=p, B=2, M=1, Lr=20, keys=p, counts=p, U=100, lrl=3.0, sigma=6.0, ignore=ign,
              n_ignore=0, mode=1, idx=None, n=2, rew=p, adv=p)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.ick_cider_d(a["cand"], a["N"], a["T"], a["refs"], a["B"], a["M"], a["Lr"], a["keys"], a["counts"],
                               a["U"], a["lrl"], a["sigma"], START, END, PAD, a["ignore"], a["n_ignore"], a["mode"],
                               a["idx"], a["n"], a["rew"], a["adv"], None)

    for bad in (dict(cand=None), dict(refs=None), dict(keys=None), dict(counts=None), dict(rew=None),
                dict(N=0), dict(T=0), dict(T=65), dict(B=0), dict(M=0), dict(M=17), dict(Lr=0), dict(Lr=65),
                dict(U=0), dict(sigma=0.0), dict(sigma=-1.0), dict(lrl=-1.0), dict(lrl=float("inf")),
                dict(n_ignore=17), dict(n_ignore=-1), dict(n_ignore=2, ignore=None), dict(mode=3), dict(mode=-1),
                dict(mode=0, idx=None), dict(adv=None), dict(n=0), dict(N=7), dict(mode=2, N=4, n=1),
                dict(mode=2, N=5), dict(n=64, N=130)):
        assert call(**bad) == -1, bad
    assert call(keys=ctypes.c_void_p(24)) == -2                         # keys not 16-byte aligned


def test_ops_wrapper_rejects_host_and_misshaped_tensors(built_lib):
    import torch
    import ick_amd.ops as ops
    from ick_amd.lib import IckError
    t = torch.zeros(4, 5, dtype=torch.int64)
    k = torch.zeros(3, 4, dtype=torch.int32)
    with pytest.raises(IckError):
        ops.cider_d(t, t.view(4, 1, 5), k, k[:, 0].contiguous(), 1.0, 6.0, START, END, PAD, baseline="greedy")
    with pytest.raises(IckError):
        ops.cider_d(t, t.view(4, 1, 5), k, k[:, 0].contiguous(), 1.0, 6.0, START, END, PAD, baseline="max")
