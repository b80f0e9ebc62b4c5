"""Restatements the reconstruction kernels (xvr_amd/csrc/recon_kernels.hip) are checked against; not collected by pytest.

* ``tv_restated``       the smoothed isotropic total variation in torch ops (slices, sqrt, sum), any dtype, with autograd;
* ``tv_grad_closed``    its gradient written out from the closed form (shifts by hand, no autograd);
* ``adam_restated``     the projected Adam update, line by line, with the non-finite-gradient rule.
"""
import math

import torch


def _forward_differences(V, weights):
    """d_a(i) = w_a (V[i + e_a] - V[i]), 0 where i + e_a is outside (Neumann)."""
    D0, D1, D2 = V.shape
    d0 = torch.cat([weights[0] * (V[1:] - V[:-1]), V.new_zeros(1, D1, D2)], dim=0)
    d1 = torch.cat([weights[1] * (V[:, 1:] - V[:, :-1]), V.new_zeros(D0, 1, D2)], dim=1)
    d2 = torch.cat([weights[2] * (V[:, :, 1:] - V[:, :, :-1]), V.new_zeros(D0, D1, 1)], dim=2)
    return d0, d1, d2


def tv_restated(V, weights=(1.0, 1.0, 1.0), eps=1e-3):
    """TV = sum_i (n(i) - eps), n(i) = sqrt(d_0^2 + d_1^2 + d_2^2 + eps^2), in V's dtype."""
    d0, d1, d2 = _forward_differences(V, weights)
    n = torch.sqrt(d0 * d0 + d1 * d1 + d2 * d2 + eps * eps)
    return (n - eps).sum()


def tv_grad_closed(V, weights=(1.0, 1.0, 1.0), eps=1e-3):
    """dTV/dV[i] = -(w_0 d_0(i) + w_1 d_1(i) + w_2 d_2(i)) / n(i) + sum_a w_a d_a(i - e_a) / n(i - e_a), terms with i - e_a
    outside dropped."""
    d = _forward_differences(V, weights)
    n = torch.sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2] + eps * eps)
    g = -(weights[0] * d[0] + weights[1] * d[1] + weights[2] * d[2]) / n
    for a in range(3):
        flux = weights[a] * d[a] / n
        back = torch.zeros_like(V)
        back.narrow(a, 1, V.shape[a] - 1).copy_(flux.narrow(a, 0, V.shape[a] - 1))
        g = g + back
    return g


def tv_value_and_grad(V, weights, eps, dtype):
    """(value, gradient) of the restatement evaluated in ``dtype`` by autograd, on the CPU."""
    x = V.detach().cpu().to(dtype).requires_grad_(True)
    val = tv_restated(x, weights, eps)
    (g,) = torch.autograd.grad(val, x)
    return val.detach(), g


def adam_restated(p, g, m, v, t, lr=1e-2, betas=(0.9, 0.999), eps=1e-8, lo=0.0, hi=math.inf, maximize=False):
    """One projected Adam step number ``t`` (1, 2, ...) in the tensors' dtype; p, m, v are updated IN PLACE.  -> how many voxels were
    skipped for a non-finite gradient (those keep p, m, v)."""
    b1, b2 = betas
    bc1, bc2 = 1.0 - b1 ** t, 1.0 - b2 ** t
    g = -g if maximize else g
    ok = torch.isfinite(g)
    gg = torch.where(ok, g, torch.zeros_like(g))
    m_new = b1 * m + (1.0 - b1) * gg
    v_new = b2 * v + (1.0 - b2) * gg * gg
    p_new = p - (lr / bc1) * m_new / (v_new.sqrt() / math.sqrt(bc2) + eps)
    p_new = torch.minimum(torch.maximum(p_new, torch.full_like(p, lo)), torch.full_like(p, hi))
    p.copy_(torch.where(ok, p_new, p))
    m.copy_(torch.where(ok, m_new, m))
    v.copy_(torch.where(ok, v_new, v))
    return int((~ok).sum())


def adam_run(p0, grads, dtype, **kw):
    """The restatement over a list of gradients from zero state, in ``dtype`` on the CPU -> (p, m, v, skipped)."""
    p = p0.detach().cpu().to(dtype).clone()
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    skipped = 0
    for t, g in enumerate(grads, start=1):
        skipped += adam_restated(p, g.detach().cpu().to(dtype), m, v, t, **kw)
    return p, m, v, skipped
