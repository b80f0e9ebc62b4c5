"""Golden vectors from small helpers of the REFERENCE, for tests/test_reference_goldens.py.

Six pieces of the reference are pinned without the reference tree at test time: the registrar's and trainer's config defaults
(``config/registrar.py``, ``config/trainer.py``), the ``Evaluator`` of ``metrics/evaluator.py``, the DRR factory
``initialize_drr`` of ``renderer/load.py``, ``_parse_scales`` of ``registrar/base.py``, the ``Standardize`` / ``Equalize``
classes of ``utils/preprocess.py`` and ``_construct_antipode`` of ``model/inference.py``.  Each runs here, unmodified, over
``xvr_amd.compat.install_as_diffdrr()`` standing in for diffdrr (loaded by path, or compiled on its own where its module
imports packages that are not installed), and what it returned -- with the arguments it handed to this package, where that
is what the test replays -- goes into ``xvr_reference_helpers.npz``.  Nothing of the reference's text is stored.

    python tests/golden/make_golden_reference_helpers.py --reference <reference checkout>/src/xvr
"""
import argparse
import ast
import importlib.util
import json
import struct
import sys
import tempfile
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))

from xvr_amd.compat import install_as_diffdrr  # noqa: E402

install_as_diffdrr(force=True)


def load(ref, relpath, name):
    spec = importlib.util.spec_from_file_location(name, ref / relpath)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def compiled(ref, relpath, kind, names, ns):
    """Only the named top-level definitions of a reference file, compiled on their own into ``ns``."""
    path = ref / relpath
    body = [n for n in ast.parse(path.read_text()).body if isinstance(n, kind) and n.name in names]
    assert {n.name for n in body} == set(names), (relpath, names)
    exec(compile(ast.Module(body=body, type_ignores=[]), str(path), "exec"), ns)
    return ns


def write_nifti(path, data, affine, dtype):
    """A minimal NIfTI-1 file (the same writer as tests/test_reference_goldens.py)."""
    hdr = bytearray(348)
    struct.pack_into("<i", hdr, 0, 348)
    struct.pack_into("<8h", hdr, 40, 3, *data.shape, 1, 1, 1, 1)
    struct.pack_into("<h", hdr, 70, {"<i2": 4, "<f4": 16}[dtype])
    struct.pack_into("<h", hdr, 72, {"<i2": 16, "<f4": 32}[dtype])
    struct.pack_into("<8f", hdr, 76, 1.0, *[float(np.linalg.norm(affine[:3, i])) for i in range(3)], 0, 0, 0, 0)
    struct.pack_into("<f", hdr, 108, 352.0)
    struct.pack_into("<2f", hdr, 112, 1.0, 0.0)
    struct.pack_into("<2h", hdr, 252, 0, 1)
    for r in range(3):
        struct.pack_into("<4f", hdr, 280 + 16 * r, *[float(x) for x in affine[r]])
    hdr[344:348] = b"n+1\0"
    with open(path, "wb") as f:
        f.write(bytes(hdr) + b"\0" * 4 + np.asfortranarray(data.astype(dtype)).tobytes(order="F"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, type=Path, help="the reference checkout's src/xvr")
    ap.add_argument("--out", type=Path, default=Path(__file__).resolve().parent / "xvr_reference_helpers.npz")
    args = ap.parse_args()
    args.scratch = Path(tempfile.mkdtemp())   # (the two NIfTI files of the factory case)
    ref = args.reference
    out = {}

    # --- config defaults
    reg = load(ref, "config/registrar.py", "xvr_ref_config_registrar").RegistrarArgs()
    keys = ("scales", "n_itrs", "parameterization", "convention", "lr_rot", "lr_xyz", "patience", "threshold", "max_n_plateaus",
            "crop", "equalize")
    tr = load(ref, "config/trainer.py", "xvr_ref_config_trainer").TrainerArgs()
    out["config_defaults"] = np.array(json.dumps({"registrar": {k: getattr(reg, k) for k in keys},
                                                  "trainer": {k: getattr(tr, k) for k in ("renderer", "batch_size", "parameterization")}}))

    # --- Evaluator over this package's DRR: mPE, mRPE, mTRE, double geodesic per (true, predicted) pair
    from xvr_amd.data import make_phantom, read
    from xvr_amd.drr import DRR
    from xvr_amd.pose import convert

    ev_mod = load(ref, "metrics/evaluator.py", "xvr_ref_evaluator")
    vol, _ = make_phantom(16, seed=1)
    drr = DRR(read(vol, orientation="AP"), 1020.0, 32, 4.0, reverse_x_axis=False)
    fid = torch.tensor([[[10.0, -5.0, 3.0], [-8.0, 6.0, -2.0], [0.0, 0.0, 12.0]]])
    g = torch.Generator().manual_seed(5)
    # the two pairs the test reads physically (identical poses; a pure 5 mm shift along the detector's columns), then four random ones
    pairs = [((0.1, 0.05, -0.02), (2.0, 700.0, -3.0), (0.1, 0.05, -0.02), (2.0, 700.0, -3.0)),
             ((0.1, 0.05, -0.02), (2.0, 700.0, -3.0), (0.1, 0.05, -0.02), (2.0, 700.0, 2.0))]
    for _ in range(4):
        r = (0.3 * torch.randn(3, generator=g)).tolist()
        t = (torch.tensor([0.0, 700.0, 0.0]) + 20 * torch.randn(3, generator=g)).tolist()
        dr = (0.05 * torch.randn(3, generator=g)).tolist()
        dt = (5 * torch.randn(3, generator=g)).tolist()
        pairs.append((r, t, [a + b for a, b in zip(r, dr)], [a + b for a, b in zip(t, dt)]))
    ev = ev_mod.Evaluator(drr, fid)
    poses = torch.tensor(pairs, dtype=torch.float32)                  # [K, 4, 3]: true rot, true xyz, predicted rot, predicted xyz
    metrics = []
    for p in poses:
        a = convert(p[0:1], p[1:2], parameterization="euler_angles", convention="ZXY")
        b = convert(p[2:3], p[3:4], parameterization="euler_angles", convention="ZXY")
        metrics.append(ev(a, b))
    out["evaluator_fiducials"] = fid.numpy()
    out["evaluator_poses"] = poses.numpy()
    out["evaluator_metrics"] = np.array(metrics, dtype=np.float64)    # [K, 4]: mPE, mRPE, mTRE, dgeo (mm)

    # --- initialize_drr on two NIfTI files: what the DRR it returns holds
    load_mod = load(ref, "renderer/load.py", "xvr_ref_renderer_load")
    rng = np.random.default_rng(0)
    hu = (rng.random((12, 14, 10)) * 2000 - 1000).astype(np.float32)
    seg = rng.integers(0, 4, size=hu.shape).astype(np.float32)
    affine = np.diag([1.5, 1.5, 2.0, 1.0])
    affine[:3, 3] = [-9.0, -10.0, -10.0]
    args.scratch.mkdir(parents=True, exist_ok=True)
    write_nifti(args.scratch / "ct.nii", hu, affine, "<f4")
    write_nifti(args.scratch / "seg.nii", seg, affine, "<i2")
    d = load_mod.initialize_drr(str(args.scratch / "ct.nii"), str(args.scratch / "seg.nii"), "1,3", "AP", 20, 24, 1020.0, 2.0, 2.5,
                                1.0, -2.0, True, "trilinear", read_kwargs={}, drr_kwargs={"voxel_shift": 0.0}, device="cpu")
    pose = convert(torch.zeros(1, 3), torch.tensor([[0.0, 800.0, 0.0]]), parameterization="euler_angles", convention="ZXY")
    src, tgt = d.detector(pose, None)
    out["factory_density"] = d.density.detach().numpy()
    out["factory_mask"] = d.mask.detach().numpy()
    out["factory_affine"] = d.affine.matrix.detach().numpy()
    out["factory_source"] = src.detach().numpy()
    out["factory_target"] = tgt.detach().numpy()

    # --- _parse_scales(scales.split(","), crop, height), as registrar/base.py calls it
    ns = compiled(ref, "registrar/base.py", ast.FunctionDef, ["_parse_scales"], {})
    cases = (("8", 0, 2048), ("8,4", 0, 2048), ("24,12,6", 100, 1436), ("4,2,1", 50, 512), ("2.5,1", 7, 999))
    out["parse_scales"] = np.array(json.dumps([[s, c, h, [float(x) for x in ns["_parse_scales"](s.split(","), c, h)]] for s, c, h in cases]))

    # --- Standardize and Equalize on random images
    ns = compiled(ref, "utils/preprocess.py", ast.ClassDef, ["Standardize", "Identity", "Equalize"], {"torch": torch})
    g = torch.Generator().manual_seed(3)
    x = torch.rand(3, 1, 24, 20, generator=g) * 7.0 - 1.0
    std = ns["Standardize"]()(x)
    out["preprocess_x"] = x.numpy()
    out["preprocess_standardize"] = std.numpy()
    out["preprocess_equalize"] = ns["Equalize"]()(std).numpy()

    # --- _construct_antipode over this package's pose module, applied twice: the Euler ZXY parameters it hands to convert
    from xvr_amd.pose import RigidTransform

    handed = []

    def spy_convert(*a, **k):
        handed.append((a[0].detach().clone(), a[1].detach().clone(), k))
        return convert(*a, **k)

    ns = compiled(ref, "model/inference.py", ast.FunctionDef, ["_construct_antipode"],
                  {"torch": torch, "RigidTransform": RigidTransform, "convert": spy_convert})
    rot = torch.tensor([[0.4, 0.2, -0.1], [2.9, -0.3, 0.05]])
    xyz = torch.tensor([[0.0, 800.0, 0.0], [0.0, 650.0, 0.0]])
    pose = convert(rot, xyz, parameterization="euler_angles", convention="ZXY")
    anti = ns["_construct_antipode"](pose)
    back = ns["_construct_antipode"](anti)
    assert len(handed) == 2 and all(k == {"parameterization": "euler_angles", "convention": "ZXY"} for *_, k in handed), handed
    out["antipode_rot"], out["antipode_xyz"] = rot.numpy(), xyz.numpy()
    out["antipode_handed_rot"] = torch.stack([h[0] for h in handed]).numpy()     # [2 (first, second call), B, 3]
    out["antipode_handed_xyz"] = torch.stack([h[1] for h in handed]).numpy()
    out["antipode_matrix"] = torch.stack([anti.matrix, back.matrix]).detach().numpy()

    np.savez_compressed(args.out, **out)
    print(f"wrote {args.out}: " + ", ".join(f"{k} {v.shape}" for k, v in out.items()))


if __name__ == "__main__":
    main()
