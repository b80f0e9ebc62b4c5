"""float16 against float32 volume storage of the trilinear forward at the C2 size (512^3 -> 256^2, B = 116, n_points = 500, the
pose-only step): pack time of the tiled copies (volume_layout 3 and 4), forward + jacobian time from fp32 tiles and from half
tiles, and the largest absolute / relative image difference between the two.  The two storages ALTERNATE in one process after a
warm-up; every figure is the median over the alternations with its spread (min .. max).  Run on the GPU box; prints a markdown
table (profiles/half_volume_bench.md records it).

    python tools/bench_half_volume.py [--size 512] [--det 256] [--batch 116] [--n-points 500] [--rounds 5] [--inner 6] [--warmup 3]
"""
import argparse
import ctypes
import statistics
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
from bench import deepfluoro_poses  # noqa: E402
from xvr_amd import _lib, renderers  # noqa: E402
from xvr_amd.data import make_phantom, read  # noqa: E402
from xvr_amd.drr import DRR  # noqa: E402


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def forward_jac_ms(drr, rot, xyz, n_points):
    """One pose-only step; -> (milliseconds of its forward + jacobian launch, from the events the binding puts around the C call,
    milliseconds of the whole step, the image)."""
    renderers.PROFILER = []
    rot.grad = xyz.grad = None

    def step():
        img = drr(rot, xyz, parameterization="euler_angles", convention="ZXY", n_points=n_points)
        img.sum().backward()
        step.img = img.detach()

    whole = event_ms(step)
    torch.cuda.synchronize()
    fwd = [a.elapsed_time(b) for name, a, b in renderers.PROFILER if name == "trilinear_forward+jac"]
    packs = [name for name, _, _ in renderers.PROFILER if name.startswith("pack")]
    renderers.PROFILER = None
    assert len(fwd) == 1 and not packs, (fwd, packs)      # (the copies were built during the warm-up)
    return fwd[0], whole, step.img


def spread(xs):
    return f"{statistics.median(xs):.3f} ({min(xs):.3f} .. {max(xs):.3f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--det", type=int, default=256)
    ap.add_argument("--batch", type=int, default=116)
    ap.add_argument("--n-points", type=int, default=500)
    ap.add_argument("--rounds", type=int, default=5, help="alternations of the two storages (at least 3)")
    ap.add_argument("--inner", type=int, default=6, help="steps per storage and alternation (their median is the alternation's figure)")
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_half_volume: needs a GPU")
    if args.rounds < 3:
        raise SystemExit("bench_half_volume: at least three alternations")
    dev = torch.device("cuda", 0)
    lib = _lib.load()
    S, H, B = args.size, args.det, args.batch
    vol, _ = make_phantom(S, n_ellipsoids=64, seed=0, device=dev)
    subject = read(vol, orientation="AP")
    delx = 1.08821875 * 256 / H
    drrs = {s: DRR(subject, 1020.0, H, delx, renderer="trilinear", reverse_x_axis=False, volume_storage=s).to(dev) for s in ("float32", "float16")}
    rot0, xyz0 = deepfluoro_poses(B, seed=0).convert("euler_angles", "ZXY")
    rot, xyz = rot0.to(dev).requires_grad_(True), xyz0.to(dev).requires_grad_(True)
    if renderers.plan_volume(drrs["float32"].renderer.make_spec(args.n_points), tuple(vol.shape), B, H * H).kind != "ypairs":
        raise SystemExit("bench_half_volume: at this size the fp32 module does not take the tiled copy; nothing to compare")

    # pack passes, alternating, each between its own pair of events
    D = tuple(vol.shape)
    bufs = {3: torch.empty(lib.xvr_drr_ytiles_bytes(*D) // 4, device=dev), 4: torch.empty(lib.xvr_drr_htiles_bytes(*D) // 4, device=dev)}
    fns = {3: lib.xvr_drr_pack_ytiles, 4: lib.xvr_drr_pack_htiles}
    pack = {3: [], 4: []}
    stream = lambda: ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)   # noqa: E731
    for r in range(args.warmup + args.rounds):
        for layout in (3, 4):
            ts = [event_ms(lambda: _lib.check(fns[layout](ctypes.c_void_p(vol.data_ptr()), *D, ctypes.c_void_p(bufs[layout].data_ptr()), stream()),
                                              "pack")) for _ in range(args.inner)]
            if r >= args.warmup:
                pack[layout].append(statistics.median(ts))
    del bufs

    fwd, whole, imgs = {s: [] for s in drrs}, {s: [] for s in drrs}, {}
    for r in range(args.warmup + args.rounds):
        for s, drr in drrs.items():
            runs = [forward_jac_ms(drr, rot, xyz, args.n_points) for _ in range(args.inner)] if r else \
                [(0.0, 0.0, drr(rot, xyz, parameterization="euler_angles", convention="ZXY", n_points=args.n_points).detach())]
            imgs[s] = runs[-1][2]
            if r >= args.warmup:
                fwd[s].append(statistics.median(t[0] for t in runs))
                whole[s].append(statistics.median(t[1] for t in runs))
    a, h = imgs["float32"], imgs["float16"]
    d = (h - a).abs()
    rel = d / a.abs().clamp_min(1e-3 * a.abs().max())
    gb = {3: lib.xvr_drr_ytiles_bytes(*D) / 2 ** 30, 4: lib.xvr_drr_htiles_bytes(*D) / 2 ** 30}
    print(f"trilinear forward, {S}^3 -> {H}^2, B = {B}, n_points = {args.n_points}, pose-only step; {args.rounds} alternations x {args.inner} "
          f"steps per storage after {args.warmup} warm-up alternations; median (min .. max) over the alternations, HIP events, ms")
    print("| what | float32 tiles (layout 3) | float16 tiles (layout 4) |")
    print("|---|---|---|")
    print(f"| copy size, GiB | {gb[3]:.3f} | {gb[4]:.3f} |")
    print(f"| pack pass | {spread(pack[3])} | {spread(pack[4])} |")
    print(f"| forward + jacobian launch | {spread(fwd['float32'])} | {spread(fwd['float16'])} |")
    print(f"| whole pose-only step | {spread(whole['float32'])} | {spread(whole['float16'])} |")
    ratio = statistics.median(fwd["float16"]) / statistics.median(fwd["float32"])
    print(f"\nforward + jacobian, half / fp32: {ratio:.3f}")
    print(f"image difference half - fp32: max |d| = {d.max().item():.4e} (image max {a.max().item():.4e}), "
          f"max |d| / max(|fp32|, 1e-3 image max) = {rel.max().item():.3e}")


if __name__ == "__main__":
    main()
