"""What the reconstruction step costs at the C2 size (512^3 -> 256^2, B = 116, n_points = 500): three legs ALTERNATING in one process
after a warm-up, HIP events around every step, random data --

  (i)   render + backward alone (the voxel gradient is computed and dropped);
  (ii)  the same + a torch-ops smoothed TV with autograd + torch.optim.Adam on the 512^3 leaf (default, and fused=True where this
        torch accepts it), clamped at 0;
  (iii) the same + xvr_amd.reconstruction.VolumeAdam with tv_weight > 0 (xvr_drr_tv_smooth + xvr_drr_volume_adam_step);

and the two new kernels on their own: time per launch, the bytes they MUST move (the step: 7 streams x 4 B per voxel; the TV:
3 x 4 B per voxel -- read V, read and write g) over that time, beside the 6.29 TB/s float4 copy rate of this chip.  Prints a markdown
report (profiles/reconstruction_bench.md records it).  Run on the GPU box:

    python tools/bench_reconstruction.py [--size 512] [--det 256] [--batch 116] [--n-points 500] [--steps 20] [--warmup 5]
"""
import argparse
import statistics
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
from bench import deepfluoro_poses  # noqa: E402
from recon_restated import tv_restated  # noqa: E402
from xvr_amd.data import read  # noqa: E402
from xvr_amd.drr import DRR  # noqa: E402
from xvr_amd.reconstruction import VolumeAdam, _tv_launch  # noqa: E402

COPY_RATE_TBS = 6.29     # float4 copy, measured (MI355X)


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def spread(xs):
    return f"{statistics.median(xs):.3f} ({min(xs):.3f} .. {max(xs):.3f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--det", type=int, default=256)
    ap.add_argument("--batch", type=int, default=116)
    ap.add_argument("--n-points", type=int, default=500)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--tv-weight", type=float, default=1e-3)
    ap.add_argument("--skip-torch", action="store_true", help="leave leg (ii) out (it needs several volume-sized temporaries)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_reconstruction: needs a GPU")
    dev = torch.device("cuda", 0)
    S, H, B = args.size, args.det, args.batch
    g = torch.Generator(device=dev).manual_seed(0)
    vol0 = torch.rand(S, S, S, device=dev, generator=g)
    drr = DRR(read(vol0, orientation="AP"), 1020.0, H, 1.08821875 * 256 / H, renderer="trilinear", reverse_x_axis=False).to(dev)
    rot0, xyz0 = deepfluoro_poses(B, seed=0).convert("euler_angles", "ZXY")
    rot, xyz = rot0.to(dev), xyz0.to(dev)
    target = torch.rand(B, 1, H, H, device=dev, generator=g)

    def render_backward(leaf):
        leaf.grad = None
        pred = drr(rot, xyz, parameterization="euler_angles", convention="ZXY", density=leaf, n_points=args.n_points)
        loss = torch.mean((pred - target) ** 2)
        return loss

    legs = {}
    leaf_i = vol0.clone().requires_grad_(True)
    legs["(i) render + backward"] = lambda: render_backward(leaf_i).backward()

    leaf_h = vol0.clone().requires_grad_(True)
    opt_h = VolumeAdam(leaf_h, lr=1e-3, tv_weight=args.tv_weight)

    def leg_hip():
        render_backward(leaf_h).backward()
        opt_h.step()
    legs["(iii) + VolumeAdam with TV (HIP)"] = leg_hip

    if not args.skip_torch:
        def torch_leg(fused):
            leaf = vol0.clone().requires_grad_(True)
            try:
                opt = torch.optim.Adam([leaf], lr=1e-3, fused=True) if fused else torch.optim.Adam([leaf], lr=1e-3)
            except (RuntimeError, TypeError, ValueError) as e:
                print(f"(torch.optim.Adam(fused=True) is not accepted here: {e})")
                return None

            def leg():
                (render_backward(leaf) + args.tv_weight * tv_restated(leaf, (1.0, 1.0, 1.0), 1e-3)).backward()
                opt.step()
                with torch.no_grad():
                    leaf.clamp_(min=0.0)
            return leg
        for name, fused in (("(ii) + torch TV + torch.optim.Adam", False), ("(ii) + torch TV + torch.optim.Adam(fused=True)", True)):
            leg = torch_leg(fused)
            if leg is not None:
                legs[name] = leg

    times = {k: [] for k in legs}
    for r in range(args.warmup + args.steps):
        for name, leg in legs.items():
            t = event_ms(leg)
            if r >= args.warmup:
                times[name].append(t)

    # the two kernels alone, alternating
    n = vol0.numel()
    gbuf = torch.randn(S, S, S, device=dev, generator=g)
    leaf_k = vol0.clone().requires_grad_(True)
    opt_k = VolumeAdam(leaf_k, lr=1e-3)
    leaf_k.grad = gbuf
    k_tv, k_tv_value_only, k_adam = [], [], []
    for r in range(args.warmup + args.steps):
        a = event_ms(lambda: _tv_launch(leaf_k.detach(), gbuf, args.tv_weight, 1e-3, (1.0, 1.0, 1.0)))
        b = event_ms(lambda: _tv_launch(leaf_k.detach(), None, args.tv_weight, 1e-3, (1.0, 1.0, 1.0)))
        c = event_ms(opt_k.step)
        if r >= args.warmup:
            k_tv.append(a)
            k_tv_value_only.append(b)
            k_adam.append(c)

    print(f"reconstruction step, trilinear, {S}^3 -> {H}^2, B = {B}, n_points = {args.n_points}, random volume / targets; {args.steps} timed "
          f"steps per leg after {args.warmup} warm-ups, the legs alternating in one process; HIP events, ms, median (min .. max)")
    print(f"device: {torch.cuda.get_device_name(0)}; torch {torch.__version__}\n")
    print("| leg | ms per step | over leg (i) |")
    print("|---|---|---|")
    base = statistics.median(times["(i) render + backward"])
    for name, ts in times.items():
        print(f"| {name} | {spread(ts)} | {statistics.median(ts) - base:+.3f} |")
    print("\n| kernel (alone, between its own events) | ms per launch | bytes it must move | achieved TB/s | share of the 6.29 TB/s copy rate |")
    print("|---|---|---|---|---|")
    for name, ts, streams in (("xvr_drr_tv_smooth, value + gradient (k_tv_smooth + k_tv_sum)", k_tv, 3),
                              ("xvr_drr_tv_smooth, value only", k_tv_value_only, 1),
                              ("xvr_drr_volume_adam_step (k_volume_adam)", k_adam, 7)):
        nbytes = streams * 4 * n
        rate = nbytes / (statistics.median(ts) * 1e-3) / 1e12
        print(f"| {name} | {spread(ts)} | {streams} x 4 B x {n} = {nbytes / 2 ** 30:.2f} GiB | {rate:.2f} | {100 * rate / COPY_RATE_TBS:.0f} % |")
    print(f"\nskipped voxels (non-finite gradients) in leg (iii): {opt_h.skipped_total()}")


if __name__ == "__main__":
    main()
