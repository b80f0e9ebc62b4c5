"""The training step's X-ray augmentations (xvr_amd/augment.py, xvr_amd/csrc/aug_kernels.hip) against their torch restatement
(tests/augment_restated.py): the parameter sampler and the noise generator on the CPU, every op and the whole chain on the GPU."""
import ctypes
import re
from pathlib import Path

import numpy as np
import pytest
import torch

import augment_restated as R

ROOT = Path(__file__).resolve().parents[1]
SIZES = [(256, 256), (200, 136), (16, 16)]


# ------------------------------------------------------------------------------------------------------------------- CPU
def test_module_exports_and_abi():
    from xvr_amd import _lib, augment

    for name in ("AugmentSpec", "XrayAugmentations", "sample_params", "apply", "clahe_luts", "standardize", "COLS", "FLAGS"):
        assert hasattr(augment, name), name
    assert _lib.ABI_VERSION == 12
    assert re.search(r"#define XVR_DRR_ABI_VERSION 12\b", (ROOT / "include" / "xvr_drr.h").read_text())
    header = (ROOT / "include" / "xvr_sim.h").read_text()
    cols = {m[0]: int(m[1]) for m in re.findall(r"#define XVR_SIM_AUG_([A-Z_]+) (\d+)", header)}
    for name, col in cols.items():
        assert getattr(augment, name) == col, name
    lib = _lib.load()
    assert lib.xvr_sim_augment_param_cols() == augment.COLS
    assert lib.xvr_sim_augment_lut_bytes(3) == 3 * 8 * 8 * 256


def test_argument_errors_are_codes():
    from xvr_amd import _lib

    lib = _lib.load()
    p = ctypes.c_void_p(16)   # (never dereferenced: every call below fails its checks first)
    assert lib.xvr_sim_augment_clahe_lut(None, p, 1, 64, 64, 0, p, None) == -1
    assert lib.xvr_sim_augment_chain(p, p, p, 0, 64, 64, 0.01, 0.0, p, None) == -1
    assert lib.xvr_sim_augment_chain(p, p, p, 1, 8, 64, 0.01, 0.0, p, None) == -3   # 8 px: the padding of 16 would exceed it
    assert b"reflect padding" in lib.xvr_drr_last_error()


def test_spec_validation():
    from xvr_amd.augment import AugmentSpec, XrayAugmentations

    AugmentSpec(clahe_clip="per_image")
    for bad in (dict(clahe_clip="last"), dict(gamma_range=(1.8, 0.7)), dict(gamma_range=(0.0, 1.0)), dict(erase_scale=(0.0, 0.3)),
                dict(erase_scale=(0.1, 1.5)), dict(std_eps=0.0), dict(noise_std=-1.0)):
        with pytest.raises(ValueError):
            AugmentSpec(**bad)
    with pytest.raises(ValueError):
        XrayAugmentations(p=1.5)
    with pytest.raises(Exception):
        AugmentSpec().noise_std = 0.1   # frozen


def test_sample_params_shapes_ranges_and_frequencies():
    from xvr_amd import augment as A

    B, H, W = 20000, 200, 136
    t = A.sample_params(B, H, W, generator=torch.Generator().manual_seed(0), p=0.333)
    assert t.shape == (B, A.COLS) and t.dtype == torch.float32 and t.device.type == "cpu"
    for c in A.FLAGS:
        assert set(t[:, c].unique().tolist()) <= {0.0, 1.0}
        assert abs(t[:, c].mean().item() - 0.333) < 0.015, c
    spec = A.AugmentSpec()
    for c, (lo, hi) in ((A.CLIP, spec.clip_range), (A.GAMMA, spec.gamma_range), (A.SHARP, spec.sharpness_range)):
        assert t[:, c].min() >= lo and t[:, c].max() <= hi
    y0, x0, h, w = (t[:, c] for c in (A.ERASE_Y, A.ERASE_X, A.ERASE_H, A.ERASE_W))
    for v in (y0, x0, h, w, t[:, A.CROP], t[:, A.SEED_LO], t[:, A.SEED_HI]):
        assert torch.equal(v, v.round())
    assert (h >= 1).all() and (w >= 1).all() and (y0 >= 0).all() and (x0 >= 0).all()
    assert (y0 + h <= H).all() and (x0 + w <= W).all()
    area = h * w / (H * W)
    assert area.median() > spec.erase_scale[0] and area.median() < spec.erase_scale[1]
    assert set(t[:, A.CROP].unique().tolist()) == set(float(k) for k in range(11))
    assert t[:, A.SEED_LO].min() >= 0 and t[:, A.SEED_HI].max() < A.SEED_BOUND
    g = torch.Generator().manual_seed(0)
    assert torch.equal(A.sample_params(B, H, W, generator=g, p=0.333), t)   # same seed, same table
    assert A.sample_params(50, H, W, generator=g, p=0.0)[:, list(A.FLAGS)].sum() == 0
    assert A.sample_params(50, H, W, generator=g, p=1.0)[:, list(A.FLAGS)].min() == 1
    same = A.sample_params(50, H, W, generator=g, same_on_batch=True)
    assert torch.equal(same, same[:1].expand(50, -1))


def test_no_cpu_path():
    from xvr_amd.augment import XrayAugmentations, apply, sample_params

    x = torch.rand(2, 1, 32, 32)
    with pytest.raises(RuntimeError, match="no CPU path"):
        XrayAugmentations()(x)
    with pytest.raises(RuntimeError, match="no CPU path"):
        apply(x, sample_params(2, 32, 32, generator=torch.Generator()))


def test_host_noise_generator():
    """Philox-4x32-10 against the Random123 known-answer vectors; the series log / cos against numpy's; the normals' moments."""
    assert [int(v) for v in R.philox4x32_10(0, 0, 0, 0, 0, 0)] == [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8]
    assert [int(v) for v in R.philox4x32_10(*[0xFFFFFFFF] * 6)] == [0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD]
    assert [int(v) for v in R.philox4x32_10(0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344, 0xA4093822, 0x299F31D0)] == \
        [0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1]
    u = np.random.default_rng(0).integers(0, 2**32, 200000).astype(np.float64) * 2.0**-32
    assert np.abs(R.aug_log(u + 2.0**-32) - np.log(u + 2.0**-32)).max() < 1e-14
    assert np.abs(R.aug_cos2pi(u) - np.cos(2 * np.pi * u)).max() < 1e-14
    y, x = np.meshgrid(np.arange(700, dtype=np.uint32), np.arange(700, dtype=np.uint32), indexing="ij")
    z = R.normal(np.uint32(123), np.uint32(456), np.uint32(3), y, x)
    assert z.dtype == np.float32 and abs(z.mean()) < 0.005 and abs(z.var() - 1) < 0.01
    assert abs(np.mean(z**3)) < 0.02 and abs(np.mean(z**4) - 3) < 0.05
    assert np.array_equal(z, R.normal(np.uint32(123), np.uint32(456), np.uint32(3), y, x))       # a pure function of its counter
    assert not np.array_equal(z, R.normal(np.uint32(124), np.uint32(456), np.uint32(3), y, x))
    assert np.array_equal(z[5:9, 7:11], R.normal(np.uint32(123), np.uint32(456), np.uint32(3), y[5:9, 7:11], x[5:9, 7:11]))


# ------------------------------------------------------------------------------------------------------------------- GPU
def _images(B, H, W, seed=0):
    """Smooth X-ray-like images with a flat background (ties in the histograms) on the GPU."""
    g = torch.Generator().manual_seed(seed)
    yy, xx = torch.meshgrid(torch.linspace(-1, 1, H), torch.linspace(-1, 1, W), indexing="ij")
    c = torch.rand(B, 4, generator=g)
    img = torch.exp(-((yy - c[:, 0, None, None] + 0.5) ** 2 + (xx - c[:, 1, None, None] + 0.5) ** 2) * (2 + 6 * c[:, 2, None, None]))
    img = img + 0.2 * torch.rand(B, H, W, generator=g) * (img > 0.3)
    return (300.0 * img.clamp(min=0.1) - 40.0)[:, None].cuda()


def _one_op(B, H, W, flag, seed=1, spec=None):
    from xvr_amd import augment as A

    t = A.sample_params(B, H, W, generator=torch.Generator().manual_seed(seed), p=1.0)
    for c in A.FLAGS:
        if c != flag:
            t[:, c] = 0.0
    return t.cuda()


def _ulps(a, b):
    return ((a.double() - b.double()).abs() / torch.finfo(torch.float32).eps).max().item()


@pytest.mark.gpu
@pytest.mark.parametrize("H,W", SIZES)
def test_clahe_luts_exact(H, W):
    from xvr_amd import augment as A

    for mode in ("first", "per_image"):
        spec = A.AugmentSpec(clahe_clip=mode)
        x = _images(6, H, W)
        t = _one_op(6, H, W, A.CLAHE)
        t[2, A.CLAHE] = 0.0        # an unselected image between selected ones
        t[0, A.CLAHE] = 0.0        # "first" is then image 1
        s = A.standardize(x, spec)
        assert torch.equal(s[:, 0], R.standardize(x))
        lut = A.clahe_luts(s, t, spec)
        clip = t[:, A.CLIP].double().cpu()
        if mode == "first":
            clip = clip[1].expand(6)
        ref = R.clahe_luts(s[:, 0].cpu(), clip)
        sel = (t[:, A.CLAHE] != 0).cpu()
        assert torch.equal(lut.cpu()[sel], ref[sel]), mode


@pytest.mark.gpu
@pytest.mark.parametrize("H,W", SIZES)
@pytest.mark.parametrize("op", ["CLAHE", "GAMMA_ON", "BLUR", "SHARP_ON", "ERASE", "CROP_ON"])
def test_each_op_alone(op, H, W):
    from xvr_amd import augment as A

    flag = getattr(A, op)
    x = _images(4, H, W, seed=2)
    t = _one_op(4, H, W, flag, seed=3)
    if op == "SHARP_ON":
        t[1, A.SHARP], t[2, A.SHARP] = 0.0, 1.0    # the two special factors
    out = A.apply(x, t)
    s = R.standardize(x)
    ref = R.chain(s.cpu(), t.cpu())
    tol = {"CLAHE": 8, "GAMMA_ON": 8, "BLUR": 8, "SHARP_ON": 16}.get(op, 0)
    assert _ulps(out[:, 0].cpu(), ref) <= tol, (op, _ulps(out[:, 0].cpu(), ref))
    if op in ("ERASE", "CROP_ON"):
        assert torch.equal(out[:, 0].cpu(), ref.float())
        assert (out == 0).sum() > 0


@pytest.mark.gpu
@pytest.mark.parametrize("H,W", SIZES)
def test_noise_bit_equal_to_host_generator(H, W):
    from xvr_amd import augment as A

    x = _images(3, H, W, seed=4)
    t = _one_op(3, H, W, A.NOISE, seed=5)
    out = A.apply(x, t)
    ref = R.chain(R.standardize(x).cpu(), t.cpu(), dtype=torch.float32)
    assert torch.equal(out[:, 0].cpu(), ref)


@pytest.mark.gpu
def test_noise_moments_full_batch():
    from xvr_amd import augment as A

    x = _images(116, 256, 256, seed=6)
    t = _one_op(116, 256, 256, A.NOISE, seed=7)
    z = (A.apply(x, t) - A.standardize(x)).double() / 0.01
    assert abs(z.mean().item()) < 2e-3 and abs(z.var().item() - 1) < 5e-3
    per_image = z.flatten(1).std(1)
    assert (per_image - 1).abs().max() < 0.02
    assert abs(torch.corrcoef(torch.stack([z[0].flatten(), z[1].flatten()]))[0, 1].item()) < 0.02


@pytest.mark.gpu
@pytest.mark.parametrize("p", [0.333, 1.0])
def test_whole_chain_c5_size(p):
    from xvr_amd import augment as A

    x = _images(116, 256, 256, seed=8)
    t = A.sample_params(116, 256, 256, generator=torch.Generator(device="cuda").manual_seed(9), p=p)
    out = A.apply(x, t)
    ref = R.chain(R.standardize(x), t)   # (on the GPU: the float64 restatement at this size)
    err = (out[:, 0].double() - ref).abs().max().item()
    assert err < 2e-5, err
    assert torch.isfinite(out).all()


@pytest.mark.gpu
def test_p_zero_is_standardize_alone():
    from xvr_amd.augment import XrayAugmentations

    x = _images(16, 200, 136, seed=10)
    out = XrayAugmentations(p=0.0)(x)
    assert torch.equal(out[:, 0], R.standardize(x))


@pytest.mark.gpu
def test_same_seed_same_bits_and_input_untouched():
    from xvr_amd.augment import XrayAugmentations

    x = _images(32, 256, 256, seed=11)
    x0 = x.clone()
    a = XrayAugmentations(p=0.5, generator=torch.Generator(device="cuda").manual_seed(5))(x)
    b = XrayAugmentations(p=0.5, generator=torch.Generator(device="cuda").manual_seed(5))(x)
    c = XrayAugmentations(p=0.5, generator=torch.Generator(device="cuda").manual_seed(6))(x)
    assert torch.equal(a, b) and not torch.equal(a, c)
    assert torch.equal(x, x0)
    assert a.shape == x.shape and a.data_ptr() != x.data_ptr()


@pytest.mark.gpu
def test_image_depends_only_on_itself_its_params_and_the_batch_range():
    from xvr_amd import augment as A

    x = _images(8, 256, 256, seed=12)
    t = A.sample_params(8, 256, 256, generator=torch.Generator(device="cuda").manual_seed(13), p=1.0)
    lo, hi = x.min(), x.max()
    y = x.clone()
    y[3] = lo + (hi - lo) * torch.rand_like(y[3])     # another image, inside the same range
    y[3, 0, 0, 0], y[3, 0, 0, 1] = lo, hi
    u = t.clone()
    u[3, A.CLIP] = 2.5                                 # (p = 1: image 0 is the first selected, its clip limit is everybody's)
    u[3, A.SEED_LO] += 1
    a, b = A.apply(x, t), A.apply(y, u)
    keep = [i for i in range(8) if i != 3]
    assert torch.equal(a[keep], b[keep])
    assert not torch.equal(a[3], b[3])


@pytest.mark.gpu
def test_forward_does_not_synchronise_and_rejects_grad():
    from xvr_amd.augment import XrayAugmentations

    x = _images(8, 128, 128, seed=14)
    aug = XrayAugmentations(generator=torch.Generator(device="cuda").manual_seed(0))
    aug(x)   # (library loaded, allocator warm)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        out = aug(x)
        out2 = XrayAugmentations(p=1.0)(x)
    finally:
        torch.cuda.set_sync_debug_mode(0)
    torch.cuda.synchronize()
    assert out.shape == out2.shape == x.shape
    with pytest.raises(RuntimeError, match="forward only"):
        aug(x.clone().requires_grad_(True))
