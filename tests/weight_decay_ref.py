"""Weight decay inside the optimizer kernels (csrc/adam.hip), restated in numpy.

    decoupled (torch.optim.AdamW)            f = 1 - lr_t * wd;   p = p * f;   then Adam's unchanged update
    coupled (torch.optim.Adam(weight_decay=))  x2 = x + wd * p feeds the moments and the update; the gradient stays x

with x = clamp(g * (gscale / den) [* coef], +-clip), the gradient after scale, clip coefficient and element clamp.

The float32 forms round after every operation, in the kernel's order: wd and lr_t are float32, one product and one
difference make f; per element one product (decoupled), or one product and one sum (coupled).  Beside them the float64
forms of the whole step for both kinds of decay."""
import numpy as np

F = np.float32


def decoupled_factor32(lr_t, wd):
    """f = 1 - lr_t * wd: one product, one difference."""
    return F(F(1.0) - F(F(lr_t) * F(wd)))


def shrink32(p, f):
    return (np.asarray(p, dtype=F) * F(f)).astype(F)


def clamped_grad32(g, den, clip, coef=None, gscale=1.0):
    """The gradient Adam consumes: g * (gscale / den) [* coef], clamped to +-clip (clip <= 0: no clamp)."""
    s = F(F(gscale) / F(den))
    x = (np.asarray(g, dtype=F) * s).astype(F)
    if coef is not None:
        x = (x * F(coef)).astype(F)
    if clip > 0:
        x = np.minimum(np.maximum(x, F(-clip)), F(clip)).astype(F)
    return x


def coupled_grad32(x, p, wd):
    """x + wd * p: the product, then the sum."""
    term = (F(wd) * np.asarray(p, dtype=F)).astype(F)
    return (np.asarray(x, dtype=F) + term).astype(F)


def adam_step64(p, g, m, v, t, lr, wd, decay, decoupled, betas=(0.9, 0.999), eps=1e-8):
    """One whole step in float64 -> (p, m, v).  g: the gradient Adam is handed (already scaled and clamped); decay: a
    bool, or a bool array like p, where the decay applies; t: the 1-based step."""
    p, g, m, v = (np.asarray(a, dtype=np.float64) for a in (p, g, m, v))
    on = np.broadcast_to(np.asarray(decay, dtype=bool), p.shape)
    b1, b2 = betas
    if decoupled:
        p = np.where(on, p * (1.0 - lr * wd), p)
    else:
        g = np.where(on, g + wd * p, g)
    m = b1 * m + (1.0 - b1) * g
    v = b2 * v + (1.0 - b2) * g * g
    step = lr / (1.0 - b1 ** t)
    p = p - step * m / (np.sqrt(v) / np.sqrt(1.0 - b2 ** t) + eps)
    return p, m, v


def adamw_step64(p, g, m, v, t, lr, wd, decay=True, **kw):
    return adam_step64(p, g, m, v, t, lr, wd, decay, True, **kw)


def adam_l2_step64(p, g, m, v, t, lr, wd, decay=True, **kw):
    return adam_step64(p, g, m, v, t, lr, wd, decay, False, **kw)
