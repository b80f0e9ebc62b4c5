"""On-device X-ray augmentations of the pose regressor's training step: the forward-only, batched equivalent of xvr's
XrayAugmentations (/root/reference/src/xvr/model/augmentations.py:7-68, a kornia AugmentationSequential applied at
/root/reference/src/xvr/model/trainer.py:207), on HIP (xvr_amd/csrc/aug_kernels.hip, include/xvr_sim.h: xvr_sim_augment_*).

The chain: Standardize over the whole batch tensor (always), then, each with probability p per image, CLAHE, gamma, 3 x 3 box
blur, Gaussian noise, sharpness, erasing, and zeroing a random border band.  kornia cannot be read or run where this was built,
so its semantics are restated as recalled; every convention that could not be pinned is a field of AugmentSpec (DESIGN.md
"Augmentations").  ``sample_params`` draws a [B, COLS] float32 table with torch's RNG, on the device; ``apply`` is
deterministic given that table.  No CPU path, no backward.
"""

from __future__ import annotations

import dataclasses

import torch

# columns of the parameter table (include/xvr_sim.h: XVR_SIM_AUG_*)
CLAHE, CLIP, GAMMA_ON, GAMMA, BLUR, NOISE, SHARP_ON, SHARP, ERASE, ERASE_Y, ERASE_X, ERASE_H, ERASE_W, CROP_ON, CROP, SEED_LO, SEED_HI = range(17)
COLS = 17
FLAGS = (CLAHE, GAMMA_ON, BLUR, NOISE, SHARP_ON, ERASE, CROP_ON)   # in the chain's order
SEED_BOUND = 1 << 24   # seeds are integers held exactly in float32


@dataclasses.dataclass(frozen=True)
class AugmentSpec:
    """The recalled constants of xvr's XrayAugmentations and the knobs for what could not be pinned (DESIGN.md "Augmentations")."""

    std_eps: float = 1e-6                      # Standardize: (x - min) / (max - min + std_eps), min / max over the batch tensor
    clip_range: tuple = (1.0, 10.0)            # RandomClahe(clip_limit=(1, 10)), grid 8 x 8, 256 bins
    clahe_clip: str = "first"                  # "first": the first selected image's clip limit for the whole selected sub-batch
                                               # (recalled kornia behaviour); "per_image": each image its own
    gamma_range: tuple = (0.7, 1.8)            # RandomGamma(gamma=(0.7, 1.8)), gain 1
    noise_std: float = 0.01                    # RandomGaussianNoise(std=0.01), mean 0, no clamp
    sharpness_range: tuple = (0.0, 0.5)        # RandomSharpness(sharpness=0.5): factor ~ U(0, 0.5)
    erase_scale: tuple = (0.02, 0.33)          # RandomErasing(scale, ratio, value)
    erase_ratio: tuple = (0.3, 3.3)
    erase_value: float = 0.0

    def __post_init__(self):
        if self.clahe_clip not in ("first", "per_image"):
            raise ValueError(f"AugmentSpec.clahe_clip must be 'first' or 'per_image', not {self.clahe_clip!r}")
        for name in ("clip_range", "gamma_range", "sharpness_range", "erase_scale", "erase_ratio"):
            lo, hi = getattr(self, name)
            if not lo <= hi:
                raise ValueError(f"AugmentSpec.{name}: lower bound above upper bound ({lo}, {hi})")
        if self.gamma_range[0] <= 0 or self.erase_ratio[0] <= 0:
            raise ValueError("AugmentSpec: gamma and the erasing aspect ratio must be positive")
        if not (0 < self.erase_scale[0] and self.erase_scale[1] <= 1):
            raise ValueError("AugmentSpec.erase_scale must lie in (0, 1]")
        if not self.std_eps > 0 or not self.noise_std >= 0:
            raise ValueError("AugmentSpec: std_eps must be positive and noise_std non-negative")


def clahe_tile(n: int) -> int:
    """CLAHE tile side for an image side of n pixels (kornia, recalled): ceil(n / 8), rounded up to even."""
    t = -(-n // 8)
    return t + (t & 1)


def check_size(H: int, W: int) -> None:
    for n in (H, W):
        if n < 2 or 8 * clahe_tile(n) - n >= n:
            raise ValueError(f"XrayAugmentations: an image side of {n} px is too small for the CLAHE tiles' reflect padding")


def sample_params(B: int, H: int, W: int, spec: AugmentSpec = AugmentSpec(), generator: torch.Generator | None = None,
                  device=None, p: float = 0.333, max_crop: int = 10, same_on_batch: bool = False) -> torch.Tensor:
    """The [B, COLS] float32 parameter table of one call, drawn with torch's RNG (``generator``, else the default one of
    ``device``) on ``device`` (default: the generator's device, else cuda).  No host synchronisation."""
    if device is None:
        device = generator.device if generator is not None else torch.device("cuda")
    n = 1 if same_on_batch else B
    u = torch.rand(n, 16, generator=generator, device=device)
    seeds = torch.randint(0, SEED_BOUND, (n, 2), generator=generator, device=device)
    flags = (u[:, :7] < p).float()

    def between(r, v):
        return r[0] + (r[1] - r[0]) * v

    # RandomErasing's rectangle (restated): area ~ U(scale) * H W; aspect ratio below or above 1 with even odds when the range
    # straddles 1; sides rounded and clamped to [1, H] / [1, W]; the corner uniform over the positions that keep it inside
    area = between(spec.erase_scale, u[:, 10]) * (H * W)
    r0, r1 = spec.erase_ratio
    if r0 < 1 < r1:
        ratio = torch.where(u[:, 11] < 0.5, between((r0, 1.0), u[:, 12]), between((1.0, r1), u[:, 12]))
    else:
        ratio = between(spec.erase_ratio, u[:, 12])
    eh = torch.sqrt(area * ratio).round().clamp(1, H)
    ew = torch.sqrt(area / ratio).round().clamp(1, W)
    cols = [None] * COLS   # (stacked from device columns: an index list would be a synchronising host -> device copy)
    for i, c in enumerate(FLAGS):
        cols[c] = flags[:, i]
    cols[CLIP] = between(spec.clip_range, u[:, 7])
    cols[GAMMA] = between(spec.gamma_range, u[:, 8])
    cols[SHARP] = between(spec.sharpness_range, u[:, 9])
    cols[ERASE_H], cols[ERASE_W] = eh, ew
    cols[ERASE_Y] = torch.minimum((u[:, 14] * (H - eh + 1)).floor(), H - eh)
    cols[ERASE_X] = torch.minimum((u[:, 13] * (W - ew + 1)).floor(), W - ew)
    cols[CROP] = (u[:, 15] * (max_crop + 1)).floor().clamp(max=max_crop)
    cols[SEED_LO], cols[SEED_HI] = seeds[:, 0].float(), seeds[:, 1].float()
    t = torch.stack(cols, 1)
    return t.expand(B, COLS).contiguous() if same_on_batch else t


def _check_input(x: torch.Tensor) -> None:
    if not x.is_cuda:
        raise RuntimeError("XrayAugmentations: CUDA images only (HIP kernels, no CPU path)")
    if x.dtype != torch.float32 or x.dim() != 4 or x.shape[1] != 1:
        raise RuntimeError("XrayAugmentations: float32 images of shape [B, 1, H, W] only")
    if x.requires_grad:
        raise RuntimeError("XrayAugmentations: forward only (xvr never differentiates through its augmentations); pass a detached tensor")
    if x.shape[0] > 65535:
        raise ValueError("XrayAugmentations: at most 65535 images per call")


def standardize(x: torch.Tensor, spec: AugmentSpec = AugmentSpec()) -> torch.Tensor:
    """(x - min) / (max - min + std_eps) over the whole tensor (xvr_sim_transform_forward, per_image = 0, mean 0, std 1)."""
    from . import _lib
    from .renderers import _ptr, _stream

    lib = _lib.load()
    B, n = x.shape[0], x[0].numel()
    xc = x.contiguous()
    if xc.data_ptr() % 16:
        xc = xc.clone()
    s = torch.empty_like(xc)
    state = torch.empty(lib.xvr_sim_transform_state_bytes(B), dtype=torch.uint8, device=x.device)
    _lib.check(lib.xvr_sim_transform_forward(_ptr(xc), B, n, 0, 0.0, 1.0, float(spec.std_eps), _ptr(s), _ptr(state), _stream()),
               "xvr_sim_transform_forward")
    return s


def _check_params(params: torch.Tensor, x: torch.Tensor) -> torch.Tensor:
    if params.shape != (x.shape[0], COLS) or params.dtype != torch.float32 or params.device != x.device:
        raise ValueError(f"XrayAugmentations: params must be float32 [{x.shape[0]}, {COLS}] on {x.device}")
    return params.contiguous()


def clahe_luts(s: torch.Tensor, params: torch.Tensor, spec: AugmentSpec = AugmentSpec()) -> torch.Tensor:
    """The CLAHE pass alone: uint8 LUTs [B, 8, 8, 256] of the standardised images ``s`` [B, 1, H, W] (rows of images whose CLAHE
    flag is clear are left unwritten)."""
    from . import _lib
    from .renderers import _ptr, _stream

    _check_input(s)
    params = _check_params(params, s)
    B, _, H, W = s.shape
    check_size(H, W)
    lib = _lib.load()
    s = s.contiguous()
    lut = torch.empty(B, 8, 8, 256, dtype=torch.uint8, device=s.device)
    _lib.check(lib.xvr_sim_augment_clahe_lut(_ptr(s), _ptr(params), B, H, W, int(spec.clahe_clip == "per_image"), _ptr(lut), _stream()),
               "xvr_sim_augment_clahe_lut")
    return lut


def apply(x: torch.Tensor, params: torch.Tensor, spec: AugmentSpec = AugmentSpec()) -> torch.Tensor:
    """The whole chain on float32 CUDA images [B, 1, H, W] with the parameter table ``params`` [B, COLS]: a new tensor of the same
    shape.  Deterministic given the table; ``x`` is not modified."""
    from . import _lib
    from .renderers import _ptr, _stream

    _check_input(x)
    params = _check_params(params, x)
    B, _, H, W = x.shape
    check_size(H, W)
    s = standardize(x, spec)
    lut = clahe_luts(s, params, spec)
    out = torch.empty_like(s)
    _lib.check(_lib.load().xvr_sim_augment_chain(_ptr(s), _ptr(params), _ptr(lut), B, H, W, float(spec.noise_std), float(spec.erase_value),
                                                 _ptr(out), _stream()), "xvr_sim_augment_chain")
    return out


class XrayAugmentations(torch.nn.Module):
    """Drop-in for xvr.model.augmentations.XrayAugmentations (transformation_matrix_mode is not applicable: intensity ops only).
    ``generator``: a torch.Generator on the images' device for reproducible draws (default: that device's default generator)."""

    def __init__(self, p: float = 0.333, max_crop: int = 10, same_on_batch: bool = False, spec: AugmentSpec = AugmentSpec(),
                 generator: torch.Generator | None = None):
        super().__init__()
        if not 0.0 <= p <= 1.0:
            raise ValueError(f"XrayAugmentations: p must be in [0, 1], not {p}")
        if max_crop < 0:
            raise ValueError("XrayAugmentations: max_crop must be non-negative")
        self.p, self.max_crop, self.same_on_batch, self.spec, self.generator = p, int(max_crop), same_on_batch, spec, generator

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        _check_input(x)
        B, _, H, W = x.shape
        params = sample_params(B, H, W, self.spec, self.generator, device=x.device, p=self.p, max_crop=self.max_crop,
                               same_on_batch=self.same_on_batch)
        return apply(x, params, self.spec)
