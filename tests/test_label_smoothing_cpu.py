"""CPU checks of label smoothing: the numpy restatement the GPU tests hold the kernel to equals torch's own criterion in
float64 (loss, mean and gradient), the new C entry refuses bad arguments before any launch, and the training script's
option and criteria."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from label_smoothing_ref import pack_rows, smoothed_ce, smoothed_ce_packed

PAD = 0


def _case():
    rng = np.random.default_rng(7)
    B, L, Vx = 4, 6, 11
    x = rng.normal(size=(B, L, Vx)) * 3.0
    caps = rng.integers(1, Vx, size=(B, L))
    caps[1, 3] = PAD                                    # a <pad> target inside a caption
    dl = np.array([5, 4, 0, 2])                         # one caption of decode length 0, one of L - 1
    return x, caps, dl


def _torch_rows(x, caps, dl):
    keep = np.arange(x.shape[1] - 1)[None, :] < dl[:, None]
    rows = torch.tensor(x[:, :-1][keep], dtype=torch.float64, requires_grad=True)
    return rows, torch.tensor(caps[:, 1:][keep]), keep


@pytest.mark.parametrize("eps", [0.0, 0.1, 0.5])
def test_restatement_is_torch_cross_entropy_with_label_smoothing(eps):
    x, caps, dl = _case()
    loss, count, d = smoothed_ce(x, caps, dl, PAD, eps)
    rows, tg, keep = _torch_rows(x, caps, dl)
    assert count == int(keep.sum()) - 1                 # the <pad> target does not count
    ref_sum = F.cross_entropy(rows, tg, ignore_index=PAD, label_smoothing=eps, reduction="sum")
    ref_mean = F.cross_entropy(rows, tg, ignore_index=PAD, label_smoothing=eps)
    assert abs(loss - ref_sum.item()) <= 1e-12 * abs(ref_sum.item())
    assert abs(loss / count - ref_mean.item()) <= 1e-12 * abs(ref_mean.item())
    ref_sum.backward()
    g = np.zeros_like(x)
    g[:, :-1][keep] = rows.grad.numpy()
    assert np.abs(d - g).max() <= 1e-12
    assert not d[2].any() and not d[1, 2].any() and not d[:, -1].any()   # target caps[1, 3]: row (1, 2)


def test_restatement_weights_and_packed_layout():
    x, caps, dl = _case()
    w = np.array([1.5, -0.75, 0.0, 2.0])
    loss1, n1, d1 = smoothed_ce(x, caps, dl, PAD, 0.1)
    loss_w, n_w, d_w = smoothed_ce(x, caps, dl, PAD, 0.1, w)
    per_caption = [smoothed_ce(x[b:b + 1], caps[b:b + 1], dl[b:b + 1], PAD, 0.1)[0] for b in range(4)]
    assert n_w == n1 and abs(loss_w - float(np.dot(w, per_caption))) < 1e-12
    assert np.allclose(d_w, d1 * w[:, None, None], rtol=0, atol=1e-15)
    rowmap = pack_rows(dl + 1, x.shape[1])
    assert rowmap.tolist() == [0, 1, 2, 3, 4, 6, 7, 8, 9, 18, 19]
    xp = x.reshape(-1, x.shape[2])[rowmap]
    loss_p, n_p, d_p = smoothed_ce_packed(xp, caps, dl + 1, PAD, 0.1, w)
    assert n_p == n_w and abs(loss_p - loss_w) < 1e-12
    assert np.array_equal(d_p, d_w.reshape(-1, x.shape[2])[rowmap])
    # every gradient row sums to w * (1 - (1 - eps) - eps) = 0
    assert np.abs(d_w.sum(-1)).max() < 1e-14


@pytest.fixture(scope="module")
def built_lib():
    import ick_amd.build as build
    return build.build()


def test_smooth_entry_refuses_bad_arguments_before_any_launch(built_lib):
    import ick_amd.lib as L
    lib = L.load()
    assert hasattr(ctypes.CDLL(built_lib), "ick_packed_ce_smooth")
    p = ctypes.c_void_p(16)          # never dereferenced: every check below fails before a launch
    ok = dict(scores=p, ld=32, caps=p, rowmap=p, count=p, dl=None, w=p, eps=p, B=2, L=3, Vx=32)

    def ce(**kw):
        a = dict(ok, **kw)
        return lib.ick_packed_ce_smooth(a["scores"], a["ld"], a["caps"], a["rowmap"], a["count"], a["dl"], a["w"],
                                        a["eps"], a["B"], a["L"], a["Vx"], PAD, p, p, p, p, None)

    for bad in (dict(eps=None), dict(scores=None), dict(caps=None), dict(rowmap=None), dict(count=None),
                dict(rowmap=None, count=None), dict(B=0), dict(B=70000), dict(L=0), dict(Vx=0), dict(ld=31)):
        assert ce(**bad) == -1, bad


def test_train_config_and_criteria():
    from ick_amd import train as tr
    assert tr.Config().label_smoothing == 0.0
    train_c, val_c = tr.make_criteria(PAD, 0.1)
    assert isinstance(train_c, torch.nn.CrossEntropyLoss) and isinstance(val_c, torch.nn.CrossEntropyLoss)
    assert train_c.label_smoothing == 0.1 and train_c.ignore_index == PAD
    assert val_c.label_smoothing == 0.0 and val_c.ignore_index == PAD      # validation: the plain negative log-likelihood
    plain, _ = tr.make_criteria(PAD)
    assert plain.label_smoothing == 0.0
    x, caps, dl = _case()
    rows, tg, _ = _torch_rows(x, caps, dl)
    loss, count, _ = smoothed_ce(x, caps, dl, PAD, 0.1)
    assert abs(train_c(rows, tg).item() - loss / count) < 1e-12
    assert abs(val_c(rows, tg).item() - smoothed_ce(x, caps, dl, PAD, 0.0)[0] / count) < 1e-12
