"""Volume reconstruction on the device: what consumes ``dL/dvoxel``.

* ``tv_smooth`` / ``tv_smooth_accumulate_`` -- the smoothed isotropic total variation, value and gradient in one HIP launch
  (xvr_drr_tv_smooth);
* ``VolumeAdam`` -- projected Adam over one float32 volume leaf, in place, one launch (xvr_drr_volume_adam_step); voxels whose
  gradient is not finite (the splats' overflow signal) are left alone and counted;
* ``Reconstruction`` -- render -> loss -> backward -> step over minibatches of views.

No CPU path: a CPU tensor raises.  Out of scope: HIP-graph capture of the loop (the step is milliseconds, not latency-bound, and the
bias corrections change every step), optimisers other than Adam, per-voxel update masks, and multi-rank reconstruction (the slab
all-reduce of xvr_amd.distributed composes with it: the gradient arrives reduced in ``.grad``).
"""

from __future__ import annotations

import ctypes
import math

import torch

from . import _lib


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _check_volume(name, t, dims=None):
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name} must be a tensor, got {type(t).__name__}")
    if t.dtype != torch.float32:
        raise ValueError(f"{name} must be float32, got {t.dtype}")
    if not t.is_contiguous():
        raise ValueError(f"{name} must be contiguous")
    if not t.is_cuda:
        raise RuntimeError(f"{name} is on {t.device}: the reconstruction kernels are HIP kernels and there is no CPU path; "
                           "move it to the GPU")
    if dims is not None and t.dim() != dims:
        raise ValueError(f"{name} must be [D0, D1, D2], got {tuple(t.shape)}")


def _check_tv_args(eps, weights):
    weights = (1.0, 1.0, 1.0) if weights is None else tuple(float(w) for w in weights)
    if len(weights) != 3:
        raise ValueError(f"weights must be three per-axis factors, got {weights!r}")
    if not eps > 0:
        raise ValueError(f"eps must be positive, got {eps!r}")
    return float(eps), weights


def _float32_bounds(lo, hi):
    """[lo, hi] as the float32 pair the kernel clamps to, rounded INWARD: a voxel clamped to hi = 0.8 must not come out as
    float32(0.8) = 0.800000012 > 0.8.  (Where no float32 lies in [lo, hi] -- lo == hi between two floats -- both round to nearest.)"""
    def inward(x, towards):
        t = torch.tensor(x, dtype=torch.float32)
        if (towards < 0 and t.item() > x) or (towards > 0 and t.item() < x):
            t = torch.nextafter(t, torch.tensor(math.copysign(math.inf, towards), dtype=torch.float32))
        return t.item()
    lo_f, hi_f = inward(lo, +1), inward(hi, -1)
    if lo_f > hi_f:
        lo_f, hi_f = torch.tensor(lo, dtype=torch.float32).item(), torch.tensor(hi, dtype=torch.float32).item()
    return lo_f, hi_f


def _tv_launch(volume, grad, weight, eps, weights, want_value=True):
    """lambda * dTV/dV is added into ``grad`` (None: value only); -> the device scalar lambda * TV (None without ``want_value``)."""
    lib = _lib.load()
    D0, D1, D2 = volume.shape
    value = ws = None
    nbytes = 0
    if want_value:
        value = torch.empty((), device=volume.device, dtype=torch.float32)
        nbytes = lib.xvr_drr_tv_smooth_workspace_bytes(D0, D1, D2)
        ws = torch.empty(nbytes // 8, device=volume.device, dtype=torch.float64)   # (no initial state: every word is written)
    with torch.cuda.device(volume.device):
        rc = lib.xvr_drr_tv_smooth(_ptr(volume), D0, D1, D2, weights[0], weights[1], weights[2], eps, float(weight), _ptr(grad),
                                   _ptr(value), _ptr(ws), nbytes, _stream())
    _lib.check(rc, "xvr_drr_tv_smooth")
    return value


def tv_smooth_accumulate_(volume, grad, weight, eps=1e-3, weights=(1.0, 1.0, 1.0)):
    """``grad += weight * dTV/dvolume`` in place (it rides on top of the render's voxel gradient) and -> the device scalar
    ``weight * TV(volume)``; one launch pair, no host synchronisation.  TV is the smoothed isotropic total variation with forward
    differences, per-axis factors ``weights`` and Neumann faces: ``sum_i sqrt(sum_a (w_a (V[i + e_a] - V[i]))^2 + eps^2) - eps``."""
    _check_volume("volume", volume, 3)
    _check_volume("grad", grad, 3)
    if grad.shape != volume.shape or grad.device != volume.device:
        raise ValueError("grad must have the volume's shape and device")
    eps, weights = _check_tv_args(eps, weights)
    value = _tv_launch(volume, grad, weight, eps, weights)
    torch.autograd.graph.increment_version(grad)   # (written through its pointer)
    return value


class _TVSmooth(torch.autograd.Function):
    @staticmethod
    def forward(ctx, volume, eps, weights):
        need = ctx.needs_input_grad[0]
        grad = torch.zeros_like(volume) if need else None
        value = _tv_launch(volume, grad, 1.0, eps, weights)
        ctx.save_for_backward(grad)
        return value

    @staticmethod
    def backward(ctx, gout):
        (grad,) = ctx.saved_tensors
        return grad * gout, None, None


def tv_smooth(volume, eps=1e-3, weights=(1.0, 1.0, 1.0)):
    """The smoothed isotropic total variation of ``volume`` [D0, D1, D2] as a scalar tensor with autograd: value and gradient come
    from one launch, the backward scales the saved gradient by the upstream scalar."""
    _check_volume("volume", volume, 3)
    eps, weights = _check_tv_args(eps, weights)
    return _TVSmooth.apply(volume, eps, weights)


class VolumeAdam:
    """Projected Adam over ONE float32 contiguous CUDA leaf, fused into a single in-place pass (seven streams: read p, g, m, v;
    write p, m, v).  After every update the voxels are clamped to [``lo``, ``hi``] (None: unbounded on that side; the float32 pair
    the kernel clamps to is rounded inward, so no voxel leaves the interval as given).  With
    ``tv_weight`` > 0, ``step()`` first adds ``tv_weight * dTV/dvolume`` into ``volume.grad`` (a second launch: the TV gradient
    reads the neighbours' OLD values, which an in-place step overwrites); ``last_tv`` then holds ``tv_weight * TV`` as a device scalar.

    A voxel whose gradient is NaN or +-inf keeps its value and its moments and is counted in ``skipped`` (a device counter;
    ``skipped_total()`` synchronises): the brick-local splats poison a voxel with NaN when a fixed-point sum overflows, and stock
    Adam would fold that into both moments for good."""

    def __init__(self, volume, lr=1e-2, betas=(0.9, 0.999), eps=1e-8, lo=0.0, hi=None, maximize=False, tv_weight=0.0, tv_eps=1e-3,
                 tv_weights=None):
        _check_volume("volume", volume)
        if not volume.is_leaf:
            raise ValueError("volume must be a leaf tensor (its .grad is what step() reads)")
        lo = -math.inf if lo is None else float(lo)
        hi = math.inf if hi is None else float(hi)
        if not lr >= 0 or not eps > 0 or not (0 <= betas[0] < 1 and 0 <= betas[1] < 1) or lo > hi or tv_weight < 0:
            raise ValueError("need lr >= 0, eps > 0, betas in [0, 1), lo <= hi, tv_weight >= 0")
        if tv_weight > 0 and volume.dim() != 3:
            raise ValueError("the TV term needs a [D0, D1, D2] volume")
        self.volume = volume
        self.lr, self.betas, self.eps = float(lr), (float(betas[0]), float(betas[1])), float(eps)
        self.lo, self.hi, self.maximize = lo, hi, bool(maximize)
        self.tv_weight = float(tv_weight)
        self.tv_eps, self.tv_weights = _check_tv_args(tv_eps, tv_weights)
        self.step_count = 0
        self.exp_avg = torch.zeros_like(volume, requires_grad=False)
        self.exp_avg_sq = torch.zeros_like(volume, requires_grad=False)
        self.skipped = torch.zeros((), device=volume.device, dtype=torch.int32)   # (the kernel adds to it as a uint32)
        self.last_tv = None

    _HYPER = ("lr", "betas", "eps", "lo", "hi", "maximize", "tv_weight", "tv_eps", "tv_weights")

    def zero_grad(self):
        """``.grad = None``: the next backward hands over a fresh buffer instead of accumulating into the old one (a pass saved)."""
        self.volume.grad = None

    def step(self):
        """One update from ``volume.grad``; -> ``tv_weight * TV`` as a device scalar (None without a TV term)."""
        vol, grad = self.volume, self.volume.grad
        if grad is None:
            raise RuntimeError("VolumeAdam.step(): volume.grad is None (run a backward first)")
        _check_volume("volume.grad", grad)
        self.last_tv = None
        if self.tv_weight > 0:
            self.last_tv = tv_smooth_accumulate_(vol.detach(), grad, self.tv_weight, self.tv_eps, self.tv_weights)
        self.step_count += 1
        t = self.step_count
        bc1, bc2 = 1.0 - self.betas[0] ** t, 1.0 - self.betas[1] ** t
        lo, hi = _float32_bounds(self.lo, self.hi)
        lib = _lib.load()
        with torch.cuda.device(vol.device):
            rc = lib.xvr_drr_volume_adam_step(_ptr(vol), _ptr(grad), _ptr(self.exp_avg), _ptr(self.exp_avg_sq), vol.numel(), self.lr,
                                              self.betas[0], self.betas[1], self.eps, bc1, bc2, lo, hi, int(self.maximize),
                                              _ptr(self.skipped), _stream())
        _lib.check(rc, "xvr_drr_volume_adam_step")
        # The kernel wrote through data_ptr(), which does not move the version counter the render-ready copies of the volume are
        # keyed on (renderers._VOLUME_CACHE): without this the next forward marches a stale tiled / bricked copy.
        torch.autograd.graph.increment_version(vol)
        return self.last_tv

    def skipped_total(self) -> int:
        """How many voxel updates were skipped for a non-finite gradient since construction (synchronises)."""
        return int(self.skipped.item()) & 0xFFFFFFFF

    def state_dict(self):
        return {"step": self.step_count, "exp_avg": self.exp_avg.clone(), "exp_avg_sq": self.exp_avg_sq.clone(),
                "skipped": self.skipped.clone(), "hyper": {k: getattr(self, k) for k in self._HYPER}}

    def load_state_dict(self, state):
        for k in ("exp_avg", "exp_avg_sq"):
            if tuple(state[k].shape) != tuple(self.volume.shape):
                raise ValueError(f"state {k} has shape {tuple(state[k].shape)}, the volume {tuple(self.volume.shape)}")
        self.step_count = int(state["step"])
        self.exp_avg.copy_(state["exp_avg"])
        self.exp_avg_sq.copy_(state["exp_avg_sq"])
        if "skipped" in state:
            self.skipped.copy_(state["skipped"])
        for k, v in state.get("hyper", {}).items():
            if k in self._HYPER:
                setattr(self, k, tuple(v) if isinstance(v, (list, tuple)) else v)


class Reconstruction:
    """Reconstruct a volume from X-rays with known poses: ``step()`` = render a minibatch of views from the current volume ->
    loss against the targets -> backward -> ``VolumeAdam.step()``.

    ``drr``: a DRR module on the GPU (either renderer); ``targets`` [B, 1, H, W]; ``rot`` [B, 3], ``xyz`` [B, 3] in
    ``parameterization`` / ``convention``.  The volume is a leaf initialised from ``init`` (default: zeros shaped like
    ``drr.density``).  ``loss``: "mse", or a callable (pred, target) -> scalar.  Remaining keywords go to ``VolumeAdam``;
    ``render_kwargs`` to the render (e.g. ``n_points``)."""

    def __init__(self, drr, targets, rot, xyz, parameterization="euler_angles", convention="ZXY", init=None, batch_size=None, loss="mse",
                 render_kwargs=None, **adam_kwargs):
        if not drr.density.is_cuda:
            raise RuntimeError("the DRR module is on the CPU: reconstruction runs on HIP kernels and there is no CPU path; move it to the GPU")
        dev = drr.density.device
        if targets.dim() != 4 or targets.shape[1] != 1 or len(rot) != len(targets) or len(xyz) != len(targets):
            raise ValueError("targets must be [B, 1, H, W] with one pose (rot [B, k], xyz [B, 3]) per view")
        if loss != "mse" and not callable(loss):
            raise ValueError("loss must be 'mse' or a callable (pred, target) -> scalar")
        self.drr = drr
        self.targets = targets.to(dev, torch.float32).contiguous()
        self.rot, self.xyz = rot.detach().to(dev, torch.float32).contiguous(), xyz.detach().to(dev, torch.float32).contiguous()
        self.parameterization, self.convention = parameterization, convention
        self.batch_size = len(targets) if batch_size is None else max(1, min(int(batch_size), len(targets)))
        self.loss = loss
        self.render_kwargs = dict(render_kwargs or {})
        start = torch.zeros_like(drr.density) if init is None else init.detach().to(dev, torch.float32).clone()
        if start.shape != drr.density.shape:
            raise ValueError(f"init has shape {tuple(start.shape)}, the module's density {tuple(drr.density.shape)}")
        self.volume = start.contiguous().requires_grad_(True)
        self.optimizer = VolumeAdam(self.volume, **adam_kwargs)
        self._next = 0

    def _batch(self):
        B, k = len(self.targets), self.batch_size
        idx = [(self._next + i) % B for i in range(k)]
        self._next = (self._next + k) % B
        if idx[-1] == idx[0] + k - 1:
            sl = slice(idx[0], idx[0] + k)
            return self.rot[sl], self.xyz[sl], self.targets[sl]
        sel = torch.tensor(idx, device=self.targets.device)
        return self.rot[sel], self.xyz[sel], self.targets[sel]

    def step(self):
        """-> (data loss, tv term) as detached device scalars (the tv term is None without ``tv_weight``)."""
        rot, xyz, target = self._batch()
        self.optimizer.zero_grad()
        pred = self.drr(rot, xyz, parameterization=self.parameterization, convention=self.convention, density=self.volume,
                        **self.render_kwargs)
        pred = pred.reshape(target.shape)
        data = torch.mean((pred - target) ** 2) if self.loss == "mse" else self.loss(pred, target)
        data.backward()
        tv = self.optimizer.step()
        return data.detach(), tv

    def run(self, n):
        """``n`` steps -> their data losses as a list of floats (one synchronisation, at the end)."""
        losses = [self.step()[0] for _ in range(int(n))]
        return torch.stack(losses).tolist() if losses else []

    def skipped_total(self) -> int:
        return self.optimizer.skipped_total()
