"""Torch restatement of the augmentation chain (xvr_amd/augment.py, xvr_amd/csrc/aug_kernels.hip) that the HIP kernels are
checked against, and the host restatement of their counter-based noise generator.  A helper module of tests/test_augment.py
(not collected by pytest); tools/bench_augment.py also runs it on the GPU as the composed-ops stand-in for kornia.

Each op is written as batched torch ops on any device.  The CLAHE lookups read the float32 standardised image (the histogram
bin floor(256 s) and the LUT index trunc(255 s) are float32 products, as in the kernel); everything after the lookups is computed
in ``dtype`` (float64 for the checker)."""

from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

from xvr_amd import augment as A

GRID, BINS = 8, 256


# --------------------------------------------------------------------------------------------------------------------------
# Philox-4x32-10 + Box-Muller: the same operations as aug_kernels.hip (IEEE double + - * / sqrt, no fused multiply-adds)
# --------------------------------------------------------------------------------------------------------------------------
def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Vectorised over numpy uint32 arrays (broadcast); returns the four uint32 output words."""
    M = np.uint64(0xFFFFFFFF)
    c = [np.asarray(v, dtype=np.uint64) & M for v in (c0, c1, c2, c3)]
    k = [np.asarray(v, dtype=np.uint64) & M for v in (k0, k1)]
    for _ in range(10):
        p0 = np.uint64(0xD2511F53) * c[0]
        p1 = np.uint64(0xCD9E8D57) * c[2]
        hi0, lo0 = p0 >> np.uint64(32), p0 & M
        hi1, lo1 = p1 >> np.uint64(32), p1 & M
        c = [hi1 ^ c[1] ^ k[0], lo1, hi0 ^ c[3] ^ k[1], lo0]
        k = [(k[0] + np.uint64(0x9E3779B9)) & M, (k[1] + np.uint64(0xBB67AE85)) & M]
    return [v.astype(np.uint32) for v in c]


_LOG_COEF = [0.047619047619047616, 0.05263157894736842, 0.058823529411764705, 0.06666666666666667, 0.07692307692307693,
             0.09090909090909091, 0.1111111111111111, 0.14285714285714285, 0.2, 0.3333333333333333, 1.0]
_COS_COEF = [-1.5619206968586225e-16, 4.779477332387385e-14, -1.1470745597729725e-11, 2.08767569878681e-09, -2.755731922398589e-07,
             2.48015873015873e-05, -0.001388888888888889, 0.041666666666666664, -0.5, 1.0]
_SIN_COEF = [-8.22063524662433e-18, 2.8114572543455206e-15, -7.647163731819816e-13, 1.6059043836821613e-10, -2.505210838544172e-08,
             2.7557319223985893e-06, -0.0001984126984126984, 0.008333333333333333, -0.16666666666666666, 1.0]
TWO_PI = 6.283185307179586


def _horner(coef, x2):
    p = np.full_like(x2, coef[0])
    for c in coef[1:]:
        p = p * x2 + c
    return p


def aug_log(u):
    """log(u) for u in (0, 1]: frexp, then 2 atanh((m - 1) / (m + 1)) as a series."""
    m, e = np.frexp(u)
    low = m < 0.7071067811865476
    m = np.where(low, m * 2.0, m)
    e = np.where(low, e - 1, e)
    s = (m - 1.0) / (m + 1.0)
    return e.astype(np.float64) * 0.6931471805599453 + (2.0 * s) * _horner(_LOG_COEF, s * s)


def aug_cos2pi(u):
    """cos(2 pi u) for u in [0, 1) from series on [-pi/4, pi/4]."""
    a = np.abs(np.where(u >= 0.5, u - 1.0, u))
    x1, x2, x3 = TWO_PI * a, TWO_PI * (0.25 - a), TWO_PI * (0.5 - a)
    c1 = _horner(_COS_COEF, x1 * x1)
    s2 = _horner(_SIN_COEF, x2 * x2) * x2
    c3 = -_horner(_COS_COEF, x3 * x3)
    return np.where(a <= 0.125, c1, np.where(a <= 0.375, s2, c3))


def normal(seed_lo, seed_hi, b, y, x):
    """z(seed, image, y, x) as float32, the kernel's noise before it is scaled by noise_std (numpy, broadcast)."""
    r = philox4x32_10(x, y, b, 0, seed_lo, seed_hi)
    u1 = (r[0].astype(np.float64) + 1.0) * 2.3283064365386963e-10
    u2 = r[1].astype(np.float64) * 2.3283064365386963e-10
    return (np.sqrt(-2.0 * aug_log(u1)) * aug_cos2pi(u2)).astype(np.float32)


def noise_field(params, H, W):
    """z for every pixel of the batch: float32 [B, H, W] (numpy)."""
    p = params.detach().cpu().numpy()
    B = p.shape[0]
    b = np.arange(B, dtype=np.uint32)[:, None, None]
    y = np.arange(H, dtype=np.uint32)[None, :, None]
    x = np.arange(W, dtype=np.uint32)[None, None, :]
    lo = p[:, A.SEED_LO].astype(np.uint32)[:, None, None]
    hi = p[:, A.SEED_HI].astype(np.uint32)[:, None, None]
    return normal(lo, hi, b, y, x)


# --------------------------------------------------------------------------------------------------------------------------
# The chain
# --------------------------------------------------------------------------------------------------------------------------
def standardize(x, eps=1e-6):
    """[B, 1, H, W] float32 -> [B, H, W]: the same float32 expression as xvr_sim_transform_forward (mean 0, std 1)."""
    x = x[:, 0]
    lo, hi = x.min(), x.max()
    return (x - lo) / ((hi - lo) + eps)


def clahe_luts(s, clip):
    """uint8 LUTs [B, 8, 8, 256] of the float32 images s [B, H, W]; clip [B] (float64 of the float32 table entry)."""
    B, H, W = s.shape
    TH, TW = A.clahe_tile(H), A.clahe_tile(W)
    padded = F.pad(s[:, None], [0, GRID * TW - W, 0, GRID * TH - H], mode="reflect")[:, 0]
    tiles = padded.reshape(B, GRID, TH, GRID, TW).permute(0, 1, 3, 2, 4).reshape(B, GRID * GRID, TH * TW)
    valid = (tiles >= 0) & (tiles <= 1)
    bins = (tiles * 256.0).clamp(0, 255).long()                       # torch.histc(bins=256, min=0, max=1)
    hist = torch.zeros(B, GRID * GRID, BINS, dtype=torch.int64, device=s.device).scatter_add_(2, bins, valid.long())
    px = TH * TW
    clip = clip.to(torch.float64).to(s.device)
    maxv = torch.floor(clip * px / BINS).clamp(min=1).long()[:, None, None]
    h = torch.minimum(hist, maxv)
    clipped = px - h.sum(-1, keepdim=True)
    h = h + clipped // BINS + (torch.arange(BINS, device=s.device) < clipped % BINS).long()
    h = torch.where((clip > 0)[:, None, None], h, hist)
    scale = torch.tensor(255.0 / px, dtype=torch.float32, device=s.device)
    return torch.floor((h.cumsum(-1).float() * scale).clamp(0, 255)).to(torch.uint8).reshape(B, GRID, GRID, BINS)


def _axis(n, T, dtype, device):
    """Per pixel row (column): the two LUT rows (columns) and the weight of the first (kornia's interpolation, recalled)."""
    half = T // 2
    i = torch.arange(n, device=device)
    sub = i // half
    t0 = ((sub - 1) // 2).clamp(0, GRID - 1)
    k = i - (2 * t0 + 1) * half
    w = (2 * half - 1 - k).to(dtype) / (2 * half - 1)
    edge = (sub == 0) | (sub >= 2 * GRID - 1)
    t0 = torch.where(sub == 0, 0, torch.where(sub >= 2 * GRID - 1, GRID - 1, t0))
    t1 = torch.where(edge, t0, t0 + 1)
    return t0, t1, torch.where(edge, torch.ones_like(w), w)


def clahe_map(s, lut, dtype=torch.float64):
    B, H, W = s.shape
    y0, y1, wy = _axis(H, A.clahe_tile(H), dtype, s.device)
    x0, x1, wx = _axis(W, A.clahe_tile(W), dtype, s.device)
    idx = (s * 255.0).long().clamp(0, BINS - 1)
    flat = lut.reshape(B, -1).to(dtype)

    def look(ty, tx):
        pos = (ty[:, None] * GRID + tx[None, :]) * BINS          # [H, W]
        return torch.gather(flat, 1, (pos[None] + idx).reshape(B, -1)).reshape(B, H, W)

    tl, tr, bl, br = look(y0, x0), look(y0, x1), look(y1, x0), look(y1, x1)
    t = tr + wx * (tl - tr)
    b = br + wx * (bl - br)
    return (b + wy[:, None] * (t - b)) / 255.0


def box_blur(v):
    p = F.pad(v[:, None], [1, 1, 1, 1], mode="reflect")
    return F.conv2d(p, torch.full((1, 1, 3, 3), 1.0 / 9.0, dtype=v.dtype, device=v.device))[:, 0]


def sharpness(v, factor):
    k = torch.tensor([[1.0, 1.0, 1.0], [1.0, 5.0, 1.0], [1.0, 1.0, 1.0]], dtype=v.dtype, device=v.device).view(1, 1, 3, 3) / 13
    deg = v.clone()
    deg[:, 1:-1, 1:-1] = F.conv2d(v[:, None], k)[:, 0].clamp(0, 1)
    f = factor.to(v.dtype).view(-1, 1, 1)
    blend = deg + (v - deg) * f
    blend = torch.where((f > 0) & (f < 1), blend, blend.clamp(0, 1))
    return torch.where(f == 0, deg, torch.where(f == 1, v, blend))


def chain(s, params, spec=A.AugmentSpec(), z=None, dtype=torch.float64, lut=None):
    """The augmented images [B, H, W] (``dtype``) from the float32 standardised images s [B, H, W] and the parameter table.
    ``z``: the unit normals of the noise [B, H, W] (default: the host generator's); ``lut``: CLAHE LUTs to use instead of
    computing them."""
    B, H, W = s.shape
    P = params.to(s.device)
    on = {c: (P[:, c] != 0).view(-1, 1, 1) for c in A.FLAGS}
    if lut is None:
        clip = P[:, A.CLIP].double()
        if spec.clahe_clip == "first":
            sel = P[:, A.CLAHE] != 0
            first = torch.argmax(sel.int())   # (the first selected image; unused when none is)
            clip = clip[first].expand(B)
        lut = clahe_luts(s, clip)
    v = s.to(dtype)
    v = torch.where(on[A.CLAHE], clahe_map(s, lut, dtype), v)
    v = torch.where(on[A.GAMMA_ON], torch.pow(v, P[:, A.GAMMA].to(dtype).view(-1, 1, 1)).clamp(0, 1), v)
    v = torch.where(on[A.BLUR], box_blur(v), v)
    if z is None:
        z = torch.from_numpy(noise_field(P, H, W))
    z = z.to(s.device)
    v = torch.where(on[A.NOISE], v + (z * np.float32(spec.noise_std)).to(dtype), v)
    v = torch.where(on[A.SHARP_ON], sharpness(v, P[:, A.SHARP]), v)
    y = torch.arange(H, device=s.device).view(1, H, 1)
    x = torch.arange(W, device=s.device).view(1, 1, W)
    r = {c: P[:, c].long().view(-1, 1, 1) for c in (A.ERASE_Y, A.ERASE_X, A.ERASE_H, A.ERASE_W, A.CROP)}
    rect = (y >= r[A.ERASE_Y]) & (y < r[A.ERASE_Y] + r[A.ERASE_H]) & (x >= r[A.ERASE_X]) & (x < r[A.ERASE_X] + r[A.ERASE_W])
    v = torch.where(on[A.ERASE] & rect, torch.full_like(v, spec.erase_value), v)
    k = r[A.CROP]
    band = (y < k) | (y >= H - k) | (x < k) | (x >= W - k)
    return torch.where(on[A.CROP_ON] & band, torch.zeros_like(v), v)
