"""CPU checks of the device caption metrics (BLEU-1..4, ROUGE-L, pointer precision / recall): the restatement
(metrics_ref.py) against hand-worked cases, argument errors of CaptionMetrics / reward() / the C entries that need no
device, and the exported symbols."""
import ctypes
import math
import os

import pytest

import metrics_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
START, END, PAD = 98, 99, 0
WM = {"<start>": START, "<end>": END, "<pad>": PAD}
V = 100                                                    # pointer ids are >= V


@pytest.fixture(scope="module")
def built_lib():
    import ick_amd.build as build
    return build.build()


def _row(ws, L=10):
    r = [START] + list(ws) + [END]
    return r + [PAD] * (L - len(r))


def _cap(cand, refs, **kw):
    return R.caption(cand, refs, START, END, PAD, **kw)


def _close(a, b, rel=1e-9):
    return abs(a - b) <= rel * abs(b)


# ------------------------------------------------------------------------------------------------ restatement
def test_hand_worked_sentence():
    r = _cap(_row([1, 2, 3, 4]), [_row([1, 2, 3, 5])])
    assert r.counts == [4, 3, 2, 1, 3, 2, 1, 0, 4, 4]
    assert R.lcs([1, 2, 3, 4], [1, 2, 3, 5]) == 3
    assert _close(r.bleu[0], 0.75) and _close(r.bleu[1], math.sqrt(0.5)) and _close(r.bleu[2], 0.25 ** (1 / 3))
    assert _close(r.bleu[3], (0.25e-15 / (1 + 1e-9)) ** 0.25, rel=1e-8)
    assert _close(r.rouge_l, 0.75, rel=1e-12)                  # P = R = 3/4


def test_clipping_takes_the_best_reference_count():
    r = _cap(_row([7, 7, 7, 7]), [_row([7, 7]), _row([7, 8, 7, 7])])
    assert r.counts[4] == 3 and r.counts[9] == 4               # correct1 = min(4, max(2, 3)); reflen: the closest
    assert r.counts[5] == 1                                    # bigram (7, 7): 3 in the candidate, at most 1 in a reference


def test_closest_length_tie_takes_the_shorter():
    r = _cap(_row([1, 2, 3, 4, 5]), [_row([1, 2, 3, 4]), _row([1, 2, 3, 4, 5, 6])])
    assert r.counts[8] == 5 and r.counts[9] == 4
    r = _cap(_row([1, 2, 3, 4, 5]), [_row([1, 2, 3, 4, 5, 6]), _row([1, 2, 3, 4])])      # either order
    assert r.counts[9] == 4


def test_brevity_factor():
    r = _cap(_row([1, 2]), [_row([1, 2, 3, 4])])
    ratio = (2 + 1e-15) / (4 + 1e-9)
    assert _close(r.bleu[0], (2 + 1e-15) / (2 + 1e-9) * math.exp(1 - 1 / ratio), rel=1e-12)
    assert r.bleu[0] < 0.4 and _close(math.exp(1 - 1 / ratio), math.exp(-1.0), rel=1e-8)
    # LCS 2: P = 1, R = 1/2
    assert _close(r.rouge_l, (1 + 1.44) * 0.5 / (0.5 + 1.44), rel=1e-12)


def test_empty_candidate_is_zero_everywhere():
    for cand in (_row([]), [END] * 10, [PAD] * 10):
        r = _cap(cand, [_row([1, 2, 3])], pointer_base=V)
        assert r.counts == [0, 0, 0, 0, 0, 0, 0, 0, 0, 3]
        assert all(b < 1e-300 for b in r.bleu) and r.rouge_l == 0.0 and r.pointers == [0, 0, 0]


def test_empty_reference():
    r = _cap(_row([1, 2, 3]), [_row([])])
    assert r.counts == [3, 2, 1, 0, 0, 0, 0, 0, 3, 0] and r.rouge_l == 0.0
    assert _close(r.bleu[0], 1e-15 / (3 + 1e-9), rel=1e-12)    # ratio > 1: no brevity factor
    r = _cap(_row([1, 2, 3]), [_row([]), _row([1, 2, 3])])     # beside a full one it changes nothing but reflen's choice
    assert r.counts[4:8] == [3, 2, 1, 0] and r.counts[9] == 3 and _close(r.rouge_l, 1.0, rel=1e-12)


def test_words_rule_no_end_and_ignore():
    # no <end>: every token counts
    r = _cap([1, 2, 3, 4], [_row([1, 2, 3, 4])])
    assert r.counts[:4] == [4, 3, 2, 1] and r.counts[4:8] == [4, 3, 2, 1]
    # nothing after <end>
    r = _cap([1, 2, END, 3, 4], [_row([1, 2, 3, 4])])
    assert r.counts[8] == 2
    # ignore closes the gap: "1 6 2" with 6 ignored has the bigram (1, 2)
    r = _cap(_row([1, 6, 2]), [_row([1, 2])], ignore=(6,))
    assert r.counts == [2, 1, 0, 0, 2, 1, 0, 0, 2, 2]
    r = _cap(_row([1, 6, 2]), [_row([1, 2])])
    assert r.counts[5] == 0                                    # without ignore the bigram is not there
    r = _cap(_row([1, PAD, 2]), [_row([1, 2])])                # <pad> closes the gap too
    assert r.counts[5] == 1


def test_pointer_counts():
    # a repeated pointer counts once; V + 2 is in one of the two references only; V + 3 is generated but not referenced
    cand = _row([1, V + 1, V + 1, V + 2, V + 3])
    refs = [_row([V + 1, 2, V + 4]), _row([V + 2, V + 1])]
    assert _cap(cand, refs, pointer_base=V).pointers == [2, 3, 3]
    assert _cap(cand, refs).pointers == [0, 0, 0]              # no pointer base: zeros
    rows = [_cap(cand, refs, pointer_base=V), _cap(_row([V + 4]), refs, pointer_base=V)]
    c = R.corpus(rows)
    assert c["pointer_precision"] == 3 / 4 and c["pointer_recall"] == 3 / 6 and c["captions"] == 2
    assert R.corpus([_cap(_row([1]), [_row([1])], pointer_base=V)])["pointer_precision"] == 0.0


def test_corpus_bleu_is_not_the_mean_of_sentence_scores():
    rows = [_cap(_row([1, 2, 3, 4]), [_row([1, 2, 3, 4])]), _cap(_row([5, 6, 7, 8, 9, 1]), [_row([5, 6, 1, 2, 3, 9])])]
    c = R.corpus(rows)
    sums = [a + b for a, b in zip(rows[0].counts, rows[1].counts)]
    assert sums == [10, 8, 6, 4, 8, 4, 2, 1, 10, 10]
    assert _close(c["Bleu_4"], (0.8 * 0.5 * (1 / 3) * 0.25) ** 0.25, rel=1e-8)
    mean4 = (rows[0].bleu[3] + rows[1].bleu[3]) / 2
    assert abs(c["Bleu_4"] - mean4) > 0.05
    assert _close(c["ROUGE_L"], (rows[0].rouge_l + rows[1].rouge_l) / 2, rel=1e-15)


def test_reward_and_advantages():
    row = _cap(_row([1, 2, 3, 4]), [_row([1, 2, 3, 5])])
    w = (2.0, 0.1, 0.2, 0.3, 0.4, 0.5)
    want = 2.0 * 1.5 + 0.1 * row.bleu[0] + 0.2 * row.bleu[1] + 0.3 * row.bleu[2] + 0.4 * row.bleu[3] + 0.5 * 0.75
    assert _close(R.reward(row, w, base=1.5), want, rel=1e-15)
    assert _close(R.reward(row, w), want - 3.0, rel=1e-15)
    assert R.advantages([1.0, 3.0, 2.0, 6.0, 0.5, 4.0], 2, 2, "greedy") == [0.5, 2.5, -2.0, 2.0]
    assert R.advantages([1.0, 3.0, 2.0, 6.0], 2, 2, "mean") == [-2.0, 2.0, -4.0, 4.0]


def test_lcs_against_nltk_or_pycocoevalcap():
    """A cross-check where one of the packages is installed (not the only pin: the hand-worked cases above are)."""
    rouge = pytest.importorskip("pycocoevalcap.rouge.rouge")
    a, b = "1 2 3 4 2 1 5".split(), "2 1 3 2 5 5 1".split()
    assert rouge.my_lcs(a, b) == R.lcs(a, b)


# ------------------------------------------------------------------------------------------------ Python arguments
def test_caption_metrics_argument_errors():
    import ick_amd
    from ick_amd.lib import IckError
    from ick_amd.metrics import CaptionMetrics, MetricReward
    assert ick_amd.CaptionMetrics is CaptionMetrics
    m = CaptionMetrics(WM, ignore=(5,), pointer_base=V)
    assert (m.start, m.end, m.pad, m.ignore, m.pointer_base, m.beta) == (START, END, PAD, (5,), V, 1.2)
    assert CaptionMetrics(WM).pointer_base == -1
    for kw in (dict(ignore=range(17)), dict(beta=0.0), dict(beta=float("nan")), dict(beta=float("inf")),
               dict(pointer_base=-1), dict(pointer_base=2 ** 31), dict(pointer_base=1.5)):
        with pytest.raises(IckError):
            CaptionMetrics(WM, **kw)
    with pytest.raises(IckError):
        CaptionMetrics({"<start>": 1})
    assert isinstance(m.reward(bleu=(0, 0, 0, 1)), MetricReward)
    assert m.reward(bleu=(0, 0, 0, 0.5), rouge_l=1).weights == (1.0, 0.0, 0.0, 0.0, 0.5, 1.0)
    for kw in (dict(), dict(cider_weight=2.0), dict(bleu=(1, 1, 1)), dict(bleu=(0, 0, 0, float("inf"))),
               dict(rouge_l=float("nan")), dict(cider=object(), rouge_l=1.0), dict(bleu="abcd"),
               dict(cider_weight=None, rouge_l=1.0)):
        with pytest.raises(IckError):
            m.reward(**kw)


def test_ops_wrappers_reject_host_and_misshaped_tensors(built_lib):
    import torch
    import ick_amd.ops as ops
    from ick_amd.lib import IckError
    from ick_amd.metrics import CaptionMetrics
    t = torch.zeros(4, 5, dtype=torch.int64)
    with pytest.raises(IckError):
        ops.caption_metrics(t, t.view(4, 1, 5), START, END, PAD, image_index=torch.arange(4))       # host tensors
    with pytest.raises(IckError):
        ops.caption_metrics(t, t.view(4, 1, 5), START, END, PAD, baseline="max")
    with pytest.raises(IckError):
        ops.caption_metric_sums(torch.zeros(4, 10, dtype=torch.int32), torch.zeros(4), torch.zeros(4, 3, dtype=torch.int32))
    m = CaptionMetrics(WM, device="cpu")
    with pytest.raises(IckError):
        m(t.float(), torch.arange(4), t)                                                             # not int64
    with pytest.raises(IckError):
        m(t, torch.arange(4), t.view(1, 1, 4, 5))


# ------------------------------------------------------------------------------------------------ C ABI
def test_header_binding_and_library_export_the_entries(built_lib):
    import ick_amd.lib as L
    with open(os.path.join(ROOT, "include", "ick_amd.h")) as f:
        hdr = f.read()
    lib = ctypes.CDLL(built_lib)
    for name, nargs in (("ick_caption_metrics", 26), ("ick_caption_metric_sums", 8)):
        assert "int %s(" % name in hdr and hasattr(lib, name)
        assert len(L.SIGNATURES[name]) == nargs and L.SIGNATURES[name][-1] is L.vp


def test_bad_arguments_are_einval_before_any_launch(built_lib):
    import ick_amd.lib as L
    lib = L.load()
    p = ctypes.c_void_p(16)              # never dereferenced: every call below fails its checks before a launch
    ign = (ctypes.c_int32 * 16)()
    w = (ctypes.c_float * 6)(1, 0, 0, 0, 1, 0)
    ok = dict(cand=p, N=6, T=20, refs=p, B=2, M=1, Lr=20, ignore=ign, n_ignore=0, beta=1.2, mode=1, idx=None, n=2,
              base=p, w=w, counts=p, bleu=p, rouge=p, ptrs=p, rew=p, adv=p)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.ick_caption_metrics(a["cand"], a["N"], a["T"], a["refs"], a["B"], a["M"], a["Lr"], START, END, PAD,
                                       a["ignore"], a["n_ignore"], V, a["beta"], a["mode"], a["idx"], a["n"], a["base"],
                                       a["w"], a["counts"], a["bleu"], a["rouge"], a["ptrs"], a["rew"], a["adv"], None)

    for bad in (dict(cand=None), dict(refs=None), dict(counts=None), dict(bleu=None), dict(rouge=None), dict(ptrs=None),
                dict(N=0), dict(T=0), dict(T=65), dict(B=0), dict(M=0), dict(M=17), dict(Lr=0), dict(Lr=65),
                dict(beta=0.0), dict(beta=float("inf")), dict(n_ignore=17), dict(n_ignore=-1),
                dict(n_ignore=2, ignore=None), dict(mode=3), dict(mode=-1), dict(mode=0, idx=None), dict(adv=None),
                dict(rew=None), dict(w=None), dict(rew=None, w=None, adv=None), dict(n=0), dict(N=7),
                dict(mode=2, N=4, n=1), dict(mode=2, N=5), dict(n=64, N=130),
                dict(w=(ctypes.c_float * 6)(1, 0, float("nan"), 0, 0, 0))):
        assert call(**bad) == -1, bad
    assert lib.ick_caption_metric_sums(p, p, p, 0, p, p, p, None) == -1
    assert lib.ick_caption_metric_sums(p, None, p, 4, p, p, p, None) == -1
