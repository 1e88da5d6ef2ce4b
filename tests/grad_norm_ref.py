"""float64 numpy restatement of the fused optimizer update with the global-norm clip: what
ick_grad_sqnorm + ick_adam_step[_derive] (with the words) compute, in torch's order --
    norm = sqrt(sum over every parameter of sum(g^2))            torch.nn.utils.clip_grad_norm_(params, m, norm_type=2)
    coef = min(1, max_norm / (norm + 1e-6))                      (max_norm None: 1)
    g    = clamp(g * coef, -clip, clip)                          (clip None or <= 0: no clamp)
    m    = b1 m + (1 - b1) g;  v = b2 v + (1 - b2) g^2           torch.optim.Adam, no weight decay, no amsgrad
    p   -= (lr / (1 - b1^t)) * m / (sqrt(v) / sqrt(1 - b2^t) + eps)
tests/test_grad_norm_cpu.py pins it to torch; the GPU tests compare the kernels with it."""
import numpy as np


def global_norm(grads):
    return float(np.sqrt(sum(float((np.asarray(g, dtype=np.float64) ** 2).sum()) for g in grads)))


def clip_coef(norm, max_norm):
    if max_norm is None:
        return 1.0
    c = max_norm / (norm + 1e-6)
    return 1.0 if c >= 1.0 else c          # (a NaN passes through, as torch.clamp(max=1.0) lets it)


def clip_adam_step(params, grads, ms, vs, t, lr, max_norm=None, clip=5.0, betas=(0.9, 0.999), eps=1e-8):
    """One update of the 1-based step t over lists of arrays -> (params, clipped grads, ms, vs, norm, coef), float64."""
    b1, b2 = betas
    norm = global_norm(grads)
    coef = clip_coef(norm, max_norm)
    bc1, bc2_sqrt = 1.0 - b1 ** t, np.sqrt(1.0 - b2 ** t)
    out = ([], [], [], [])
    for p, g, m, v in zip(params, grads, ms, vs):
        p, g, m, v = (np.asarray(a, dtype=np.float64) for a in (p, g, m, v))
        g = g * coef
        if clip is not None and clip > 0:
            g = np.clip(g, -clip, clip)
        m = b1 * m + (1.0 - b1) * g
        v = b2 * v + (1.0 - b2) * g * g
        p = p - (lr / bc1) * m / (np.sqrt(v) / bc2_sqrt + eps)
        for lst, a in zip(out, (p, g, m, v)):
            lst.append(a)
    return out + (norm, coef)
