"""Vectors produced by the REFERENCE's own files (src/xvr/model/sampler.py, src/xvr/model/loss.py), executed in
the build container over the diffdrr compat shim (tests/golden/make_golden_xvr.py).  They pin xvr's own
logic -- the pose sampling recipe, the Dice definition, the loss assembly and the multiview pairing."""
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

GOLD = np.load(Path(__file__).resolve().parent / "golden" / "xvr_reference_sampler_loss.npz")


def test_get_random_pose_matches_the_reference_sampler():
    from xvr_amd.training import get_random_pose

    ranges = dict(zip((str(k) for k in GOLD["sampler_keys"]), GOLD["sampler_ranges"].tolist()))
    ranges["batch_size"] = int(ranges["batch_size"])
    torch.manual_seed(123)
    mine = get_random_pose(**ranges).matrix.numpy()
    assert np.allclose(mine, GOLD["sampler_matrix"], atol=1e-5)
    # sanity of the recipe itself: sources sit ty mm from the isocentre, looking back at it
    assert (np.linalg.norm(mine[:, :3, 3], axis=1) >= 450 - 1e-3).all()


def test_oracle_loss_matches_the_reference_loss_module():
    """oracle/loss_restated.py against the vectors the reference's own loss.py produced (tests/golden/make_golden_xvr.py)."""
    from oracle import loss_restated as oloss

    t = lambda k: torch.from_numpy(GOLD[k])  # noqa: E731
    res = oloss.pose_regression_loss(t("in_img"), t("in_mask").float(), t("in_pose"), t("in_pred_img"), t("in_pred_mask").float(),
                                     t("in_pred_pose"), 1020.0, weight_mvc=1e-3)
    for k, v in zip(("loss", "mncc", "dgeo", "rgeo", "tgeo", "dice", "mvc"), res):
        assert np.allclose(v.detach().numpy(), GOLD[f"loss_{k}"], rtol=1e-5, atol=1e-5), k
    d = oloss.dice_metric(t("in_mask").float(), t("in_pred_mask").float()).numpy()
    assert np.allclose(d, GOLD["dice_metric"], equal_nan=True)
    assert np.isnan(GOLD["dice_metric"][0, 1])  # the structure that is empty in both masks


@pytest.mark.gpu
def test_pose_regression_loss_matches_the_reference_loss_module():
    """The product's loss (HIP entry points) against the same vectors."""
    from xvr_amd.loss import DiceMetric, PoseRegressionLoss
    from xvr_amd.pose import RigidTransform

    t = lambda k: torch.from_numpy(GOLD[k]).cuda()  # noqa: E731
    fn = PoseRegressionLoss(1020.0, weight_mvc=1e-3)
    res = fn(t("in_img"), t("in_mask").bool(), RigidTransform(t("in_pose")), t("in_pred_img"), t("in_pred_mask").bool(),
             RigidTransform(t("in_pred_pose")))
    for k, v in zip(("loss", "mncc", "dgeo", "rgeo", "tgeo", "dice", "mvc"), res):
        assert np.allclose(v.detach().cpu().numpy(), GOLD[f"loss_{k}"], rtol=2e-4, atol=2e-4), k
    d = DiceMetric()(t("in_mask").bool(), t("in_pred_mask").bool()).cpu().numpy()
    assert np.allclose(d, GOLD["dice_metric"], equal_nan=True)


def test_compat_shim_exposes_the_diffdrr_names_xvr_imports():
    saved = {k: v for k, v in sys.modules.items() if k == "diffdrr" or k.startswith("diffdrr.")}
    try:
        from xvr_amd.compat import install_as_diffdrr

        assert install_as_diffdrr(force=True)
        from diffdrr.data import read, transform_hu_to_density  # noqa: F401
        from diffdrr.drr import DRR  # noqa: F401
        from diffdrr.metrics import (DoubleGeodesicSE3, GradientNormalizedCrossCorrelation2d,  # noqa: F401
                                     MultiscaleNormalizedCrossCorrelation2d)
        from diffdrr.pose import RigidTransform, convert, make_matrix  # noqa: F401
        from diffdrr.registration import N_ANGULAR_COMPONENTS, Registration  # noqa: F401

        import xvr_amd.drr

        assert DRR is xvr_amd.drr.DRR and N_ANGULAR_COMPONENTS["quaternion_adjugate"] == 10
    finally:
        for k in [k for k in sys.modules if k == "diffdrr" or k.startswith("diffdrr.")]:
            del sys.modules[k]
        sys.modules.update(saved)


# Six helpers of the reference pinned by what they returned, run over the compat shim (tests/golden/make_golden_reference_helpers.py):
# the config defaults, the Evaluator, the DRR factory, _parse_scales, Standardize / Equalize and _construct_antipode.
HELPERS = np.load(Path(__file__).resolve().parent / "golden" / "xvr_reference_helpers.npz")


def test_registrar_defaults_equal_the_reference_config():
    """xvr_amd.registrar.Registrar's defaults are the reference's RegistrarArgs (src/xvr/config/registrar.py)."""
    import inspect
    import json

    from xvr_amd.registrar import Registrar

    ref = json.loads(str(HELPERS["config_defaults"]))
    mine = {k: v.default for k, v in inspect.signature(Registrar.__init__).parameters.items() if v.default is not inspect._empty}
    for key in ("scales", "n_itrs", "parameterization", "convention", "lr_rot", "lr_xyz", "patience", "threshold",
                "max_n_plateaus", "crop", "equalize"):
        assert mine[key] == ref["registrar"][key], key
    tr = ref["trainer"]
    assert tr["renderer"] == "trilinear" and tr["batch_size"] == 116 and tr["parameterization"] == "quaternion_adjugate"


def _evaluate(drr, fiducials, true_pose, pred_pose):
    """mPE (on the detector, in mm), mRPE, mTRE and the double geodesic (eps 0) of a predicted pose against the true one, through
    this package's DRR and pose surface -- the four numbers of the reference's Evaluator (src/xvr/metrics/evaluator.py)."""
    from xvr_amd.metrics import DoubleGeodesicSE3

    p_pred, p_true = drr.perspective_projection(pred_pose, fiducials), drr.perspective_projection(true_pose, fiducials)
    mpe = (drr.detector.delx * (p_pred - p_true)).norm(dim=-1).mean(dim=-1)
    mrpe = (drr.inverse_projection(pred_pose, p_pred) - drr.inverse_projection(true_pose, p_true)).norm(dim=-1).mean(dim=-1)
    mtre = (pred_pose(fiducials) - true_pose(fiducials)).norm(dim=-1).mean(dim=-1)
    dgeo = DoubleGeodesicSE3(drr.detector.sdd, eps=0.0)(true_pose, pred_pose)[2]
    return torch.stack([mpe, mrpe, mtre, dgeo], dim=-1).squeeze().tolist()


def test_reference_evaluator_runs_on_this_drr():
    """The reference's own Evaluator (src/xvr/metrics/evaluator.py: mPE, mRPE, mTRE, double geodesic) imports only
    diffdrr; run unmodified over the compat shim against this package's DRR (CPU-side geometry only), it returned the stored
    numbers, and this package's surface still gives them."""
    from xvr_amd.data import make_phantom, read
    from xvr_amd.drr import DRR
    from xvr_amd.pose import convert

    vol, _ = make_phantom(16, seed=1)
    drr = DRR(read(vol, orientation="AP"), 1020.0, 32, 4.0, reverse_x_axis=False)
    fiducials = torch.from_numpy(HELPERS["evaluator_fiducials"])
    assert fiducials.tolist() == [[[10.0, -5.0, 3.0], [-8.0, 6.0, -2.0], [0.0, 0.0, 12.0]]]
    poses = torch.from_numpy(HELPERS["evaluator_poses"])
    results = []
    for p, want in zip(poses, HELPERS["evaluator_metrics"]):
        true = convert(p[0:1], p[1:2], parameterization="euler_angles", convention="ZXY")
        pred = convert(p[2:3], p[3:4], parameterization="euler_angles", convention="ZXY")
        got = _evaluate(drr, fiducials, true, pred)
        assert np.allclose(got, want, rtol=1e-4, atol=1e-3), (p.tolist(), got, want.tolist())
        results.append(want)
    same, (mpe, mrpe, mtre, dgeo) = results[0], results[1]
    assert poses[0, 0].tolist() == poses[0, 2].tolist() and poses[0, 1].tolist() == poses[0, 3].tolist()
    assert all(abs(x) < 1e-3 for x in same), same
    # a pure 5 mm shift along the detector's column direction: mTRE = 5 mm exactly, mPE ~ 5 mm x magnification
    assert (poses[1, 3] - poses[1, 1]).tolist() == [0.0, 0.0, 5.0] and poses[1, 0].tolist() == poses[1, 2].tolist()
    assert abs(mtre - 5.0) < 1e-3 and abs(dgeo - 5.0) < 1e-2
    assert 5.0 < mpe < 5.0 * 1020.0 / 600.0 and mrpe > 0


def test_reference_initialize_drr_runs_over_the_shim(tmp_path):
    """The reference's own DRR factory (src/xvr/renderer/load.py: read(volume, mask, labels, orientation) ->
    DRR(subject, sdd, height, delx, width, dely, x0, y0, reverse_x_axis=, renderer=, **drr_kwargs).to(device))
    ran unmodified over the compat shim on these NIfTI files; the shim's read and DRR, called with the factory's arguments,
    hand back this package's DRR holding what the factory's did, with the surface xvr touches afterwards (trainer.py:251-256,
    registrar/base.py:155-212)."""
    import struct

    saved = {k: v for k, v in sys.modules.items() if k == "diffdrr" or k.startswith("diffdrr.")}
    try:
        from xvr_amd.compat import install_as_diffdrr

        install_as_diffdrr(force=True)
        from diffdrr.data import read
        from diffdrr.drr import DRR as ShimDRR

        def write_nifti(path, data, affine, dtype):
            hdr = bytearray(348)
            struct.pack_into("<i", hdr, 0, 348)
            struct.pack_into("<8h", hdr, 40, 3, *data.shape, 1, 1, 1, 1)
            struct.pack_into("<h", hdr, 70, {"<i2": 4, "<f4": 16}[dtype])
            struct.pack_into("<h", hdr, 72, {"<i2": 16, "<f4": 32}[dtype])
            struct.pack_into("<8f", hdr, 76, 1.0, *[float(np.linalg.norm(affine[:3, i])) for i in range(3)], 0, 0, 0, 0)
            struct.pack_into("<f", hdr, 108, 352.0)
            struct.pack_into("<2f", hdr, 112, 1.0, 0.0)
            struct.pack_into("<2h", hdr, 252, 0, 1)           # qform 0, sform 1
            for r in range(3):
                struct.pack_into("<4f", hdr, 280 + 16 * r, *[float(x) for x in affine[r]])
            hdr[344:348] = b"n+1\0"
            with open(path, "wb") as f:
                f.write(bytes(hdr) + b"\0" * 4 + np.asfortranarray(data.astype(dtype)).tobytes(order="F"))

        rng = np.random.default_rng(0)
        hu = (rng.random((12, 14, 10)) * 2000 - 1000).astype(np.float32)
        seg = rng.integers(0, 4, size=hu.shape).astype(np.float32)
        affine = np.diag([1.5, 1.5, 2.0, 1.0])
        affine[:3, 3] = [-9.0, -10.0, -10.0]
        write_nifti(tmp_path / "ct.nii", hu, affine, "<f4")
        write_nifti(tmp_path / "seg.nii", seg, affine, "<i2")
        # initialize_drr(ct, seg, "1,3", "AP", 20, 24, 1020.0, 2.0, 2.5, 1.0, -2.0, True, "trilinear", read_kwargs={},
        #                drr_kwargs={"voxel_shift": 0.0}, device="cpu"), as the factory passes it on
        subject = read(str(tmp_path / "ct.nii"), str(tmp_path / "seg.nii"), [1, 3], "AP")
        drr = ShimDRR(subject, 1020.0, 20, 2.0, 24, 2.5, 1.0, -2.0, reverse_x_axis=True, renderer="trilinear", voxel_shift=0.0).to("cpu")
        from xvr_amd.drr import DRR

        assert isinstance(drr, DRR) and drr.renderer.renderer_name == "trilinear" and drr.renderer.voxel_shift == 0.0
        assert (drr.detector.height, drr.detector.width, drr.detector.delx, drr.detector.dely) == (20, 24, 2.0, 2.5)
        assert tuple(drr.density.shape) == hu.shape and float(drr.density.min()) >= 0.0
        assert set(np.unique(drr.mask.numpy()).tolist()) <= {0.0, 1.0, 3.0}      # labels="1,3" keeps only those structures
        assert np.allclose(drr.density.numpy(), HELPERS["factory_density"], rtol=1e-6, atol=1e-6)
        assert np.array_equal(drr.mask.numpy(), HELPERS["factory_mask"])
        assert np.allclose(drr.affine.matrix.numpy(), HELPERS["factory_affine"], atol=1e-6)
        from xvr_amd.pose import convert

        pose = convert(torch.zeros(1, 3), torch.tensor([[0.0, 800.0, 0.0]]), parameterization="euler_angles", convention="ZXY")
        src, tgt = drr.detector(pose, None)
        assert src.shape == (1, 1, 3) and tgt.shape == (1, 20 * 24, 3)
        assert np.allclose(src.numpy(), HELPERS["factory_source"], atol=1e-4) and np.allclose(tgt.numpy(), HELPERS["factory_target"], atol=1e-4)
        drr.rescale_detector_(0.5)
        assert (drr.detector.height, drr.detector.width) == (10, 12)
    finally:
        for k in [k for k in sys.modules if k == "diffdrr" or k.startswith("diffdrr.")]:
            del sys.modules[k]
        sys.modules.update(saved)


def test_parse_scales_equals_the_reference_function():
    """registrar/base.py cannot be imported (matplotlib, torchvision, ...), but its pure helper `_parse_scales` ran on its own
    over the split list the reference passes (base.py:152); xvr_amd.registrar.parse_scales gives what it returned, call by call."""
    import json

    import pytest

    from xvr_amd.registrar import parse_scales

    cases = json.loads(str(HELPERS["parse_scales"]))
    assert [c[:3] for c in cases[:4]] == [["8", 0, 2048], ["8,4", 0, 2048], ["24,12,6", 100, 1436], ["4,2,1", 50, 512]]
    for scales, crop, height, want in cases:
        assert parse_scales(scales, crop, height) == pytest.approx(want, rel=1e-12), (scales, crop, height)


def test_standardize_and_equalize_equal_the_reference_classes():
    """utils/preprocess.py imports torchvision, but its Standardize / Equalize classes are plain torch: run on their own on
    random images, their outputs are stored, and the oracle's restatement (the checker of the HIP kernels,
    tests/test_pose_opt.py::test_equalize_hip_matches_the_torch_formulation_value_and_gradient) reproduces them."""
    from oracle import metrics_restated as mref

    g = torch.Generator().manual_seed(3)
    x = torch.rand(3, 1, 24, 20, generator=g) * 7.0 - 1.0
    assert torch.equal(x, torch.from_numpy(HELPERS["preprocess_x"]))
    std, eq = torch.from_numpy(HELPERS["preprocess_standardize"]), torch.from_numpy(HELPERS["preprocess_equalize"])
    assert torch.allclose(mref.xray_transforms(x, 24, 20), (std - 0.15) / 0.1, rtol=1e-6, atol=1e-6)
    assert torch.allclose(mref.equalize(std), eq, rtol=1e-5, atol=1e-6)
    assert torch.allclose(mref.xray_transforms(x, 24, 20, equalize_=True), (eq - 0.15) / 0.1, rtol=1e-5, atol=1e-5)


def test_reference_antipode_helper_puts_the_source_on_the_other_side():
    """model/inference.py:_construct_antipode (pure diffdrr.pose calls), run on its own over this package's pose module, read
    the pose's Euler ZXY angles and handed new ones to `convert` (stored, for two applications).  For a C-arm pose
    (xyz = (0, d, 0)) the result must carry the source to the far side of the patient -- (x, y, z) -> (x, -y, -z), a half turn
    about the left-right axis -- which only happens if the translation is applied in the camera frame, x_world = R (x_cam + t):
    the convention xvr_amd.pose.convert was pinned on (with x_world = R x_cam + t the source would not move at all).  Applying
    it twice is the identity."""
    from xvr_amd.pose import convert

    rot, xyz = torch.from_numpy(HELPERS["antipode_rot"]), torch.from_numpy(HELPERS["antipode_xyz"])
    assert torch.allclose(rot, torch.tensor([[0.4, 0.2, -0.1], [2.9, -0.3, 0.05]])) and xyz.tolist() == [[0.0, 800.0, 0.0], [0.0, 650.0, 0.0]]
    pose = convert(rot, xyz, parameterization="euler_angles", convention="ZXY")
    # what the helper read from the pose it was given: this package's conversion back to Euler ZXY
    _, t0 = pose.convert("euler_angles", "ZXY")
    handed_rot, handed_xyz = torch.from_numpy(HELPERS["antipode_handed_rot"]), torch.from_numpy(HELPERS["antipode_handed_xyz"])
    assert torch.allclose(t0, handed_xyz[0], atol=1e-3)
    anti = convert(handed_rot[0], handed_xyz[0], parameterization="euler_angles", convention="ZXY")
    assert torch.allclose(anti.matrix, torch.from_numpy(HELPERS["antipode_matrix"][0]), atol=1e-4)
    src, src_anti = pose.matrix[:, :3, 3], anti.matrix[:, :3, 3]          # camera origin in world coordinates
    assert torch.allclose(src_anti, src * torch.tensor([1.0, -1.0, -1.0]), atol=1e-3), (src, src_anti)
    assert torch.allclose(src.norm(dim=1), xyz[:, 1], atol=1e-3)           # the source orbits at distance d
    back = convert(handed_rot[1], handed_xyz[1], parameterization="euler_angles", convention="ZXY")
    assert torch.allclose(back.matrix, torch.from_numpy(HELPERS["antipode_matrix"][1]), atol=1e-4)
    assert torch.allclose(back.matrix, pose.matrix, atol=1e-4)
