"""Volume reconstruction (xvr_amd/reconstruction.py, csrc/recon_kernels.hip): the smoothed TV and the fused projected Adam step
against their restatements (tests/recon_restated.py), the version bump the render-ready copies depend on, and the loop.

Tolerances are yardsticks measured in the test itself: the distance of the FLOAT32 evaluation of a restatement from its float64
evaluation on the same input, times 4 (a different association of the same terms, not a wrong term).  Every measured distance is
printed (pytest -s) and recorded in profiles/reconstruction_bench.md."""
import ctypes
import math
import re
import sys
from pathlib import Path

import pytest
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(Path(__file__).resolve().parent))
import recon_restated as rr  # noqa: E402

gpu = pytest.mark.gpu
NEW_ENTRY_POINTS = ("xvr_drr_tv_smooth", "xvr_drr_tv_smooth_workspace_bytes", "xvr_drr_volume_adam_step")


# ------------------------------------------------------------------------------------------------ CPU
def test_header_and_binding_declare_the_entry_points_and_the_abi_version_stays_12():
    from xvr_amd import _lib

    header = (ROOT / "include" / "xvr_drr.h").read_text()
    text = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in NEW_ENTRY_POINTS:
        assert re.search(rf"\b{name}\s*\(", text), name
        assert name in _lib.EXPORTS, name
    assert re.search(r"#define\s+XVR_DRR_ABI_VERSION\s+12\b", header) and _lib.ABI_VERSION == 12
    # the prototypes agree with the declarations in length (pointer / scalar kinds are exercised by the calls below)
    for name in NEW_ENTRY_POINTS:
        decl = re.search(rf"\b{name}\s*\(([^)]*)\)", text).group(1)
        assert len(_lib.EXPORTS[name][0]) == len([a for a in decl.split(",") if a.strip()]), name


@pytest.mark.parametrize("shape", [(3, 4, 5), (2, 2, 2)])
def test_restated_tv_gradient_equals_the_closed_form_in_float64(shape):
    g = torch.Generator().manual_seed(7)
    for weights, eps in (((1.0, 1.0, 1.0), 1e-3), ((0.5, 1.25, 2.0), 1.0)):
        V = torch.rand(*shape, generator=g, dtype=torch.float64)
        _, auto = rr.tv_value_and_grad(V, weights, eps, torch.float64)
        assert (auto - rr.tv_grad_closed(V, weights, eps)).abs().max().item() <= 1e-12
        const = torch.full(shape, 0.37, dtype=torch.float64)
        val, grad = rr.tv_value_and_grad(const, weights, eps, torch.float64)
        assert val.item() == 0.0 and grad.abs().max().item() == 0.0


def test_restated_adam_equals_torch_adam_with_a_clamp_in_float64():
    g = torch.Generator().manual_seed(3)
    p0 = torch.rand(9, 10, 11, generator=g, dtype=torch.float64)
    grads = [torch.randn(9, 10, 11, generator=g, dtype=torch.float64) for _ in range(5)]
    for maximize in (False, True):
        p, m, v, skipped = rr.adam_run(p0, grads, torch.float64, lr=0.05, lo=0.0, hi=0.8, maximize=maximize)
        q = p0.clone().requires_grad_(True)
        opt = torch.optim.Adam([q], lr=0.05, maximize=maximize)
        for gr in grads:
            q.grad = gr.clone()
            opt.step()
            with torch.no_grad():
                q.clamp_(0.0, 0.8)
        assert skipped == 0 and (p - q.detach()).abs().max().item() <= 1e-12
        assert (m - opt.state[q]["exp_avg"]).abs().max().item() <= 1e-12 and (v - opt.state[q]["exp_avg_sq"]).abs().max().item() <= 1e-12


def test_no_cpu_path_and_wrong_dtype_or_layout_are_refused():
    from xvr_amd.reconstruction import VolumeAdam, tv_smooth, tv_smooth_accumulate_

    v = torch.rand(4, 5, 6)
    for call in (lambda: tv_smooth(v), lambda: VolumeAdam(v.clone().requires_grad_(True)), lambda: tv_smooth_accumulate_(v, torch.zeros_like(v), 1.0)):
        with pytest.raises(RuntimeError, match="no CPU path"):
            call()
    for bad in (v.double(), v.transpose(0, 2)):
        for call in (lambda: tv_smooth(bad), lambda: VolumeAdam(bad.clone(memory_format=torch.preserve_format).requires_grad_(True))):
            with pytest.raises(ValueError):
                call()


def test_argument_errors_of_the_new_entry_points_are_codes_with_a_message():
    from xvr_amd import _lib

    lib = _lib.load()
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    tv = lib.xvr_drr_tv_smooth
    for args, word in (((None, 4, 4, 4, 1, 1, 1, 1e-3, 1.0, p, None, None, 0, None), b"null"),
                       ((p, 4, 4, 4, 1, 1, 1, 1e-3, 1.0, None, None, None, 0, None), b"null"),
                       ((p, 4, 1, 4, 1, 1, 1, 1e-3, 1.0, p, None, None, 0, None), b"at least 2"),
                       ((p, 4, 4, 4, 1, 1, 1, 0.0, 1.0, p, None, None, 0, None), b"eps"),
                       ((p, 4, 4, 4, 1, 1, 1, 1e-3, 1.0, p, p, None, 0, None), b"workspace")):
        rc = tv(*args)
        assert rc == -1 and word in lib.xvr_drr_last_error(), (args, rc, lib.xvr_drr_last_error())
    adam = lib.xvr_drr_volume_adam_step
    ok = dict(lr=0.01, b1=0.9, b2=0.999, eps=1e-8, bc1=0.1, bc2=0.001, lo=0.0, hi=1.0)

    def call(vol=p, grad=p, m=p, v=p, n=16, **kw):
        a = {**ok, **kw}
        return adam(vol, grad, m, v, n, a["lr"], a["b1"], a["b2"], a["eps"], a["bc1"], a["bc2"], a["lo"], a["hi"], 0, None, None)

    for kw, word in ((dict(vol=None), b"null"), (dict(grad=None), b"null"), (dict(m=None), b"null"), (dict(v=None), b"null"),
                     (dict(n=0), b"n must be positive"), (dict(eps=0.0), b"eps"), (dict(lo=0.5, hi=0.25), b"lo > hi"), (dict(bc1=0.0), b"bc1")):
        rc = call(**kw)
        assert rc == -1 and word in lib.xvr_drr_last_error(), (kw, rc, lib.xvr_drr_last_error())
    with pytest.raises(RuntimeError, match="lo > hi"):
        _lib.check(call(lo=1.0, hi=0.0), "xvr_drr_volume_adam_step")
    assert lib.xvr_drr_tv_smooth_workspace_bytes(0, 4, 4) == 0 and lib.xvr_drr_tv_smooth_workspace_bytes(5, 6, 7) % 8 == 0


# ------------------------------------------------------------------------------------------------ GPU: the TV
TV_SHAPES = [(2, 2, 2), (5, 6, 7), (17, 9, 33), (16, 16, 16)]
LAMBDA = 0.3


@gpu
@pytest.mark.parametrize("shape", TV_SHAPES)
@pytest.mark.parametrize("weights", [(1.0, 1.0, 1.0), (0.5, 1.25, 2.0)])
@pytest.mark.parametrize("eps", [1e-3, 1.0])
def test_tv_matches_the_float64_restatement_within_four_float32_distances(shape, weights, eps):
    from xvr_amd.reconstruction import _tv_launch, tv_smooth_accumulate_

    g = torch.Generator().manual_seed(sum(shape) + int(10 * weights[2]))
    V = torch.rand(*shape, generator=g)
    grad0 = torch.randn(*shape, generator=g)
    val64, g64 = rr.tv_value_and_grad(V, weights, eps, torch.float64)
    val32, g32 = rr.tv_value_and_grad(V, weights, eps, torch.float32)
    want_val, want_grad = LAMBDA * val64, grad0.double() + LAMBDA * g64
    # the yardsticks: float32 restatement against float64, gradient absolute, value relative to the value
    yard_grad = ((grad0 + LAMBDA * g32).double() - want_grad).abs().max().item()
    yard_val = abs((LAMBDA * val32).double().item() - want_val.item()) / abs(want_val.item())
    acc = grad0.cuda()
    val = tv_smooth_accumulate_(V.cuda(), acc, LAMBDA, eps, weights)
    err_grad = (acc.cpu().double() - want_grad).abs().max().item()
    err_val = abs(val.double().item() - want_val.item()) / abs(want_val.item())
    only = _tv_launch(V.cuda(), None, LAMBDA, eps, weights)
    print(f"tv {shape} w={weights} eps={eps}: gradient err {err_grad:.3e} (float32 restatement {yard_grad:.3e}), "
          f"value rel.err {err_val:.3e} (float32 restatement {yard_val:.3e})")
    assert err_grad <= 4 * yard_grad
    assert err_val <= 4 * yard_val
    assert only.item() == val.item()                       # the value-only call
    again = grad0.cuda()
    val2 = tv_smooth_accumulate_(V.cuda(), again, LAMBDA, eps, weights)
    assert torch.equal(again, acc) and val2.item() == val.item()     # identical bits on a second call


@gpu
@pytest.mark.parametrize("shape", TV_SHAPES)
def test_tv_of_a_constant_volume_is_exactly_zero(shape):
    from xvr_amd.reconstruction import tv_smooth_accumulate_

    for weights, eps in (((1.0, 1.0, 1.0), 1e-3), ((0.5, 1.25, 2.0), 1.0)):
        V = torch.full(shape, 0.37, device="cuda")
        acc = torch.zeros(shape, device="cuda")
        val = tv_smooth_accumulate_(V, acc, LAMBDA, eps, weights)
        assert val.item() == 0.0 and acc.abs().max().item() == 0.0


@gpu
def test_tv_autograd_form_equals_the_accumulate_form_and_scales_with_the_upstream_scalar():
    from xvr_amd.reconstruction import tv_smooth, tv_smooth_accumulate_

    V = torch.rand(17, 9, 33, generator=torch.Generator().manual_seed(5)).cuda()
    acc = torch.zeros_like(V)
    val = tv_smooth_accumulate_(V, acc, 1.0)
    a = V.clone().requires_grad_(True)
    out = tv_smooth(a)
    out.backward()
    assert out.dim() == 0 and out.item() == val.item() and torch.equal(a.grad, acc)
    b = V.clone().requires_grad_(True)
    (3 * tv_smooth(b)).backward()
    assert torch.equal(b.grad, 3 * acc)
    assert tv_smooth(V).requires_grad is False


# ------------------------------------------------------------------------------------------------ GPU: the step
ADAM_SHAPE = (9, 10, 11)          # 990 voxels: 247 float4 and a scalar tail of 2
ADAM_KW = dict(lr=0.05, lo=0.0, hi=0.8)
_ADAM_CACHE = {}


def _adam_case(maximize):
    """p0, five gradients, and the restatement's float64 / float32 runs (computed once per direction, shared, left unchanged)."""
    if maximize not in _ADAM_CACHE:
        g = torch.Generator().manual_seed(11)
        p0 = torch.rand(*ADAM_SHAPE, generator=g)
        grads = [torch.randn(*ADAM_SHAPE, generator=g) for _ in range(5)]
        ref = rr.adam_run(p0, grads, torch.float64, maximize=maximize, **ADAM_KW)
        f32 = rr.adam_run(p0, grads, torch.float32, maximize=maximize, **ADAM_KW)
        yard = [(a.double() - b).abs().max().item() for a, b in zip(f32[:3], ref[:3])]
        _ADAM_CACHE[maximize] = (p0, grads, ref, yard)
    return _ADAM_CACHE[maximize]


def _run_volume_adam(p0, grads, **kw):
    from xvr_amd.reconstruction import VolumeAdam

    p = p0.clone().cuda().requires_grad_(True)
    opt = VolumeAdam(p, **kw)
    for gr in grads:
        p.grad = gr.clone().cuda()
        opt.step()
    return p.detach().cpu(), opt.exp_avg.cpu(), opt.exp_avg_sq.cpu(), opt


@gpu
@pytest.mark.parametrize("maximize", [False, True])
def test_adam_matches_the_float64_restatement_within_four_float32_distances(maximize):
    p0, grads, ref, yard = _adam_case(maximize)
    p, m, v, opt = _run_volume_adam(p0, grads, maximize=maximize, **ADAM_KW)
    for name, got, want, y in zip("pmv", (p, m, v), ref[:3], yard):
        err = (got.double() - want).abs().max().item()
        print(f"adam maximize={maximize} {name}: err {err:.3e} (float32 restatement {y:.3e})")
        assert err <= 4 * y, name
    assert p.min().item() >= 0.0 and p.max().item() <= 0.8
    assert opt.skipped_total() == 0


@gpu
def test_adam_first_step_with_unit_gradient_moves_every_voxel_by_lr():
    p0 = torch.full(ADAM_SHAPE, 0.5)
    p, _, _, _ = _run_volume_adam(p0, [torch.ones(ADAM_SHAPE)], lr=0.05, lo=None, hi=None)
    assert ((0.5 - p.double()) / 0.05 - 1.0).abs().max().item() <= 1e-6


@gpu
def test_adam_skips_and_counts_non_finite_gradients():
    from xvr_amd.reconstruction import VolumeAdam

    p0, grads, _, _ = _adam_case(False)
    n = p0.numel()
    planted = {0: math.nan, n - 1: math.inf, n - 2: -math.inf, 5: math.inf, 501: math.nan, 640: -math.inf}   # n - 1, n - 2: the scalar tail
    bad = [gr.clone() for gr in grads[:2]]
    for gr in bad:
        for i, val in planted.items():
            gr.view(-1)[i] = val
    idx = torch.tensor(sorted(planted))
    p = p0.clone().cuda().requires_grad_(True)
    opt = VolumeAdam(p, **ADAM_KW)
    opt.exp_avg.copy_(torch.full(ADAM_SHAPE, 0.125))      # (state that a skipped voxel must keep bit for bit)
    opt.exp_avg_sq.copy_(torch.full(ADAM_SHAPE, 0.25))
    before = [t.detach().clone() for t in (p, opt.exp_avg, opt.exp_avg_sq)]
    clean = p0.clone().cuda().requires_grad_(True)
    opt_clean = VolumeAdam(clean, **ADAM_KW)
    opt_clean.exp_avg.copy_(before[1])
    opt_clean.exp_avg_sq.copy_(before[2])
    for k, gr in enumerate(bad):
        p.grad = gr.cuda()
        opt.step()
        clean.grad = grads[k].cuda()
        opt_clean.step()
        assert opt.skipped_total() == len(planted) * (k + 1)
    keep = torch.ones(n, dtype=torch.bool)
    keep[idx] = False
    for got, was, other in zip((p.detach(), opt.exp_avg, opt.exp_avg_sq), before, (clean.detach(), opt_clean.exp_avg, opt_clean.exp_avg_sq)):
        got, was, other = got.cpu().view(-1), was.cpu().view(-1), other.cpu().view(-1)
        assert torch.equal(got[idx].view(torch.int32), was[idx].view(torch.int32))     # untouched, bit for bit
        assert torch.equal(got[keep], other[keep])                                     # every other voxel: the step without the plants
    assert opt_clean.skipped_total() == 0
    # ... and that step is the one held to the restatement (from zero state, two steps)
    p2, m2, v2, _ = _run_volume_adam(p0, bad, **ADAM_KW)
    ref = rr.adam_run(p0, bad, torch.float64, **ADAM_KW)
    f32 = rr.adam_run(p0, bad, torch.float32, **ADAM_KW)
    assert ref[3] == 2 * len(planted)
    for name, got, want, lo in zip("pmv", (p2, m2, v2), ref[:3], f32[:3]):
        assert (got.double() - want).abs().max().item() <= 4 * (lo.double() - want).abs().max().item(), name


@gpu
def test_state_dict_round_trip_is_bit_equal_to_an_uninterrupted_run():
    from xvr_amd.reconstruction import VolumeAdam

    g = torch.Generator().manual_seed(23)
    p0 = torch.rand(5, 6, 7, generator=g)
    grads = [torch.randn(5, 6, 7, generator=g) for _ in range(5)]
    kw = dict(lr=0.05, lo=0.0, hi=0.8, tv_weight=1e-2)

    def steps(opt, p, gs):
        for gr in gs:
            p.grad = gr.clone().cuda()
            opt.step()

    a = p0.clone().cuda().requires_grad_(True)
    opt_a = VolumeAdam(a, **kw)
    steps(opt_a, a, grads[:3])
    state = opt_a.state_dict()
    a2 = a.detach().clone().requires_grad_(True)
    opt_a2 = VolumeAdam(a2)                                 # (default hyper-parameters: the state carries the real ones)
    opt_a2.load_state_dict(state)
    steps(opt_a2, a2, grads[3:])
    b = p0.clone().cuda().requires_grad_(True)
    opt_b = VolumeAdam(b, **kw)
    steps(opt_b, b, grads)
    assert opt_a2.step_count == 5 and opt_a2.tv_weight == 1e-2 and opt_a2.hi == 0.8
    assert torch.equal(a2.detach(), b.detach()) and torch.equal(opt_a2.exp_avg, opt_b.exp_avg) and torch.equal(opt_a2.exp_avg_sq, opt_b.exp_avg_sq)


# ------------------------------------------------------------------------------------------------ GPU: with the renderers
def _small_drr(shape, renderer, n_views, seed=2):
    """A phantom, a DRR module of the C1 geometry scaled down to it (32^2 detector, the volume fills the view) and ``n_views``
    poses spread over 180 degrees of yaw."""
    from xvr_amd.data import make_phantom, read
    from xvr_amd.drr import DRR

    vol, _ = make_phantom(shape, n_ellipsoids=6, seed=seed)
    scale = max(shape) / 512.0
    drr = DRR(read(vol, orientation="AP"), 1020.0 * scale, 32, 1.3 * max(shape) / 24.0, renderer=renderer, reverse_x_axis=False).cuda()
    yaw = math.pi + math.pi * torch.arange(n_views, dtype=torch.float32) / n_views
    rot = torch.stack([yaw, torch.zeros(n_views), torch.zeros(n_views)], dim=1).cuda()
    xyz = torch.tensor([[0.0, 725.0 * scale, 0.0]]).repeat(n_views, 1).cuda()
    return vol, drr, rot, xyz


@gpu
@pytest.mark.parametrize("renderer", ["trilinear", "siddon"])
def test_the_render_after_a_step_sees_the_new_volume(renderer, monkeypatch):
    from xvr_amd import renderers
    from xvr_amd.reconstruction import VolumeAdam

    # (every launch is "large": the tiled y-pair copy / the bricked copy is built at first sight and cached on the tensor)
    monkeypatch.setattr(renderers, "YPAIR_FIRST_SIGHT_SAMPLES_PER_VOXEL", 0.0)
    monkeypatch.setattr(renderers, "YPAIR_MIN_WAVEFRONTS", 1)
    vol, drr, rot, xyz = _small_drr((24, 20, 28), renderer, 4)
    kw = dict(parameterization="euler_angles", convention="ZXY", **({"n_points": 48} if renderer == "trilinear" else {}))
    leaf = vol.clone().cuda().requires_grad_(True)
    opt = VolumeAdam(leaf, lr=0.05)
    with torch.no_grad():
        for _ in range(3):
            before = drr(rot, xyz, density=leaf, **kw)
    slot = renderers._VOLUME_CACHE.get(id(leaf))
    kind = "ypairs" if renderer == "trilinear" else "bricks"
    assert slot is not None and slot.get(kind) is not None and slot[kind][1] is not None, "no layout copy was cached: the test would prove nothing"
    assert before.abs().max().item() > 0
    leaf.grad = torch.randn(leaf.shape, generator=torch.Generator().manual_seed(1)).cuda()
    version = leaf._version
    opt.step()
    assert leaf._version > version
    with torch.no_grad():
        after = drr(rot, xyz, density=leaf, **kw)
        fresh = drr(rot, xyz, density=leaf.detach().clone().requires_grad_(True), **kw)
    assert torch.equal(after, fresh)
    assert not torch.equal(after, before)


def _torch_loop(drr, targets, rot, xyz, steps, batch_size, lr, tv_weight, render_kw):
    """The yardstick loop: torch.optim.Adam + the float32 torch TV with autograd through the same renderer and view order."""
    vol = torch.zeros_like(drr.density).requires_grad_(True)
    opt = torch.optim.Adam([vol], lr=lr)
    losses, B = [], len(targets)
    for k in range(steps):
        sl = slice((k * batch_size) % B, (k * batch_size) % B + batch_size)
        opt.zero_grad(set_to_none=True)
        pred = drr(rot[sl], xyz[sl], parameterization="euler_angles", convention="ZXY", density=vol, **render_kw).reshape(targets[sl].shape)
        data = torch.mean((pred - targets[sl]) ** 2)
        (data + tv_weight * rr.tv_restated(vol, (1.0, 1.0, 1.0), 1e-3)).backward()
        opt.step()
        with torch.no_grad():
            vol.clamp_(min=0.0)
        losses.append(data.detach())
    return torch.stack(losses).tolist(), vol.detach()


@gpu
@pytest.mark.parametrize("renderer", ["trilinear", "siddon"])
def test_reconstruction_loop_tracks_the_torch_loop(renderer):
    from xvr_amd.reconstruction import Reconstruction

    truth, drr, rot, xyz = _small_drr((24, 24, 24), renderer, 8)
    render_kw = {"n_points": 64} if renderer == "trilinear" else {}
    with torch.no_grad():
        targets = drr(rot, xyz, parameterization="euler_angles", convention="ZXY", **render_kw)
    assert targets.shape == (8, 1, 32, 32) and (targets > 0).float().mean().item() > 0.3
    lr, steps = 0.02, 30
    want, _ = _torch_loop(drr, targets, rot, xyz, steps, 4, lr, 1e-3, render_kw)
    rec = Reconstruction(drr, targets, rot, xyz, batch_size=4, lr=lr, tv_weight=1e-3, render_kwargs=render_kw)
    got = rec.run(steps)
    first, last = sum(want[:2]) / 2, sum(want[-2:]) / 2        # (two consecutive steps = one pass over the eight views)
    print(f"loop {renderer}: torch loop {first:.4e} -> {last:.4e}; HIP loop final {sum(got[-2:]) / 2:.4e} (last step {got[-1]:.4e} vs {want[-1]:.4e})")
    assert last <= 0.5 * first, "the yardstick loop does not converge: change lr, not this assertion"
    assert abs(got[-1] - want[-1]) <= 0.02 * want[-1]
    assert rec.skipped_total() == 0
    assert rec.volume.min().item() >= 0.0
    assert rec.optimizer.last_tv is not None and rec.optimizer.last_tv.item() > 0


@gpu
def test_float16_storage_refuses_the_voxel_gradient_unchanged():
    from xvr_amd.data import make_phantom, read
    from xvr_amd.drr import DRR
    from xvr_amd.reconstruction import Reconstruction

    vol, _ = make_phantom(16, n_ellipsoids=4, seed=1)
    drr = DRR(read(vol, orientation="AP"), 40.0, 16, 2.0, renderer="trilinear", reverse_x_axis=False, volume_storage="float16").cuda()
    rot, xyz = torch.tensor([[math.pi, 0.0, 0.0]]).cuda(), torch.tensor([[0.0, 28.0, 0.0]]).cuda()
    rec = Reconstruction(drr, torch.zeros(1, 1, 16, 16), rot, xyz, render_kwargs={"n_points": 16})
    with pytest.raises(NotImplementedError, match="float16"):
        rec.step()
