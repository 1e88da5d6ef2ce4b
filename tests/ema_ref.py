"""The exponential moving average of the parameters that the optimizer kernels keep (csrc/adam.hip),
restated in numpy.

    d_t = decay                                  without warmup
    d_t = min(decay, (1 + t) / (10 + t))         with it, t the 1-based optimizer step
    e   = e + (1 - d_t) * (p_new - e)

The float32 forms round after every operation, in the kernel's order: the decay word is a float32, (1 + t) and (10 + t)
are float32 sums, one division, one minimum, w = 1 - d_t, then per element one difference, one product, one sum.  Beside
them the float64 forms of the same expressions."""
import numpy as np

F = np.float32


def decay_at32(t, decay, warmup=False):
    d = F(decay)
    if warmup:
        t = F(t)
        d = min(d, (F(1.0) + t) / (F(10.0) + t))
    return F(d)


def decay_at64(t, decay, warmup=False):
    d, t = float(decay), float(t)
    return min(d, (1.0 + t) / (10.0 + t)) if warmup else d


def ema_update32(e, p, t, decay, warmup=False):
    """The average after optimizer step t made the parameters p: float32 arrays in, a new float32 array out."""
    e, p = np.asarray(e, dtype=F), np.asarray(p, dtype=F)
    w = F(F(1.0) - decay_at32(t, decay, warmup))
    diff = (p - e).astype(F)
    prod = (w * diff).astype(F)
    return (e + prod).astype(F)


def ema_update64(e, p, t, decay, warmup=False):
    e, p = np.asarray(e, dtype=np.float64), np.asarray(p, dtype=np.float64)
    return e + (1.0 - decay_at64(t, decay, warmup)) * (p - e)


def ema_fold32(e0, snapshots, decay, warmup=False, first_step=1):
    """The average after the steps first_step, first_step + 1, ... left the parameters snapshots[0], snapshots[1], ..."""
    e = np.asarray(e0, dtype=F)
    for i, p in enumerate(snapshots):
        e = ema_update32(e, p, first_step + i, decay, warmup)
    return e
