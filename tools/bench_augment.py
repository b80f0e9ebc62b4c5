"""Time the training step's X-ray augmentations at C5 size (B = 116 images of 256 x 256, p = 0.333) with HIP events: the HIP chain
(xvr_amd.augment.XrayAugmentations: Standardize + CLAHE LUT pass + chain pass) against the torch restatement of the same chain
(tests/augment_restated.py) run on the GPU in float32 as the composed-ops stand-in for kornia.  Run on the GPU box; writes the
table to stdout (profiles/augment_bench.md records it).

    python tools/bench_augment.py [--batch 116] [--size 256] [--iters 200] [--warmup 20]
"""
import argparse
import statistics
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
import augment_restated as R  # noqa: E402
from xvr_amd import augment as A  # noqa: E402


def timed(fn, iters, warmup):
    """Per-call milliseconds: median and min over `iters` calls, each between its own pair of events."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return statistics.median(times), min(times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=116)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_augment: needs a GPU")
    B, H = args.batch, args.size
    g = torch.Generator(device="cuda").manual_seed(0)
    x = torch.rand(B, 1, H, H, device="cuda", generator=g) * 1000.0
    aug = A.XrayAugmentations(generator=g)
    spec = A.AugmentSpec()
    params = A.sample_params(B, H, H, spec, generator=g)
    s = A.standardize(x, spec)

    def restated():   # the same chain as composed torch ops (float32), its noise from torch.randn as kornia draws it
        p = A.sample_params(B, H, H, spec, generator=g)
        st = R.standardize(x)
        return R.chain(st, p, spec, z=torch.randn(B, H, H, device="cuda", generator=g), dtype=torch.float32)

    rows = [
        ("HIP XrayAugmentations.forward (sample + standardize + LUT + chain)", timed(lambda: aug(x), args.iters, args.warmup)),
        ("HIP apply (standardize + LUT + chain, fixed table)", timed(lambda: A.apply(x, params, spec), args.iters, args.warmup)),
        ("HIP CLAHE LUT pass alone", timed(lambda: A.clahe_luts(s, params, spec), args.iters, args.warmup)),
        ("torch restatement, float32 (sample + chain)", timed(restated, max(args.iters // 10, 5), 3)),
    ]
    mb = 2 * B * H * H * 4 / 1e6
    print(f"augmentations, B = {B}, {H} x {H}, p = 0.333 ({mb:.1f} MB image in + out); per call, HIP events")
    print("| what | median ms | min ms |")
    print("|---|---|---|")
    for name, (med, mn) in rows:
        print(f"| {name} | {med:.4f} | {mn:.4f} |")


if __name__ == "__main__":
    main()
