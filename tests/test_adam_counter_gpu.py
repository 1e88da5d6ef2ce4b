"""The step counter's advance inside the optimizer launch (ick_adam_step[_derive]) against today's two
launches (the Adam entry, then ick_counter_add_if): a bucket of 4 096 + 12 floats with one item (a 64 x 64 matrix with a
plain and a transposed image, then a flat run of 12 floats), three steps and a step without a token.  Parameters,
gradients, moments, images and the counter are compared bit for bit after every step, in the flat and the cover form."""
import ctypes

import pytest
import torch

import ick_amd.lib as L
import ick_amd.ops as ops

pytestmark = pytest.mark.gpu

N = 4096 + 12


class Cover:
    """One item + one flat run over the bucket, laid out as weights.DerivedWeights hands it to ops.adam_update."""

    def __init__(self):
        self.copy = torch.zeros(64, 64, device="cuda")
        self.tr = torch.zeros(64, 64, device="cuda")
        item = L.AdamItem(off=0, rows=64, K=64, drow0=0, Nd=64, pack=None, pack_t=None, copy=self.copy.data_ptr(), ps=None,
                          ps_t=None, tr=self.tr.data_ptr(), copy_ld=64, tr_ld=64)
        blocks = (L.AdamBlock * 2)(L.AdamBlock(item=0, tn=0, tk=0, cnt4=0, off4=0, copy=None),
                                   L.AdamBlock(item=-1, tn=0, tk=0, cnt4=3, off4=1024, copy=None))
        self.items_dev = self._dev(item)
        self.blocks_dev = self._dev(blocks)
        self.n_blocks, self.nbytes = 2, 7 * 4 * N

    @staticmethod
    def _dev(obj):
        raw = ctypes.string_at(ctypes.addressof(obj), ctypes.sizeof(obj))
        return torch.frombuffer(bytearray(raw), dtype=torch.uint8).cuda()

    def images(self):
        return [self.copy, self.tr]


def state(seed):
    g = torch.Generator().manual_seed(seed)
    p = torch.randn(N, generator=g).cuda()
    m = (torch.randn(N, generator=g) * 0.01).cuda()
    v = (torch.rand(N, generator=g) * 1e-3).cuda()
    return p, m, v


@pytest.mark.parametrize("form", ["flat", "cover"])
def test_three_steps_and_a_step_without_a_token(form):
    legs = []
    for fused in (False, True):
        p, m, v = state(3)
        cover = Cover() if form == "cover" else None
        counter = torch.full((1,), 4, dtype=torch.int32, device="cuda")
        ticket = ops.adam_ticket("cuda")
        trail = []
        for i, tokens in enumerate([7.0, 5.0, 0.0, 3.0]):
            g = (torch.randn(N, generator=torch.Generator().manual_seed(50 + i)) * 40.0).cuda()
            den = torch.full((1,), tokens, device="cuda")
            kw = dict(lr=4e-4, clip=5.0, gscale=1.0, beta1=0.9, beta2=0.999, eps=1e-8, step_tensor=counter, gscale_den=den,
                      cover=cover)
            if fused:
                ops.adam_update(p, g, m, v, 1, bump=(1, ticket), **kw)
            else:
                ops.adam_update(p, g, m, v, 1, **kw)
                ops.counter_add_if(counter, 1, den)
            torch.cuda.synchronize()
            trail.append([t.clone() for t in [p, g, m, v, counter] + (cover.images() if cover else [])])
            assert int(ticket.item()) == 0
        legs.append(trail)
    for i, (a, b) in enumerate(zip(*legs)):
        for x, y, name in zip(a, b, ("p", "g", "m", "v", "counter", "copy", "tr")):
            assert torch.equal(x, y), (form, "step %d" % i, name)
    counts = [int(t[4].item()) for t in legs[1]]
    assert counts == [5, 6, 6, 7]                                   # the step without a token leaves the counter
    same = [torch.equal(x, y) for k, (x, y) in enumerate(zip(legs[1][1], legs[1][2])) if k != 1]
    assert all(same), same                                          # ... and everything else (k == 1: the new gradient)
    if form == "cover":
        assert torch.equal(legs[1][3][5].view(-1), legs[1][3][0][:4096]) and \
            torch.equal(legs[1][3][6], legs[1][3][0][:4096].view(64, 64).t())
