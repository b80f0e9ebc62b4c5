"""configs[3] in miniature across 2 ranks (gloo, both on cuda:0): sharded multi-start registration."""
import re
import subprocess
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]


@pytest.mark.gpu
def test_multistart_registration_two_ranks():
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", "29533", str(ROOT / "tools" / "register_multistart.py"), "--backend", "gloo", "--single-device",
           "--starts", "3"]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-3000:]
    # (two processes write to one pipe: a report can land behind another line's text instead of on a line of its own)
    found = list(re.finditer(r"rank \d/2: refined (\d+) starts; best ncc ([\d.]+) from rank (\d); pose error ([\d.]+) mm = ([\d.]+) deg, "
                             r"([\d.]+) mm across / ([\d.]+) mm along", out.stdout))
    assert len(found) == 2, out.stdout
    assert sorted(int(m.group(1)) for m in found) == [1, 2]                      # 3 starts split 2 + 1
    assert len({(m.group(2), m.group(3), m.group(4)) for m in found}) == 1          # every rank agrees on the winner
    # starts are 100+ mm off (+-10 degrees, +-20 mm).  The device-resident loop is bit-reproducible, so the bound is what a
    # registration should deliver (the full-size C4 test's bar): under a degree, under 2 mm across the view; a single view fixes
    # the depth poorly (1 % of magnification per 7 mm at 700 mm), hence the looser bound along it
    ncc, rot_deg, across, along = (float(found[0].group(k)) for k in (2, 5, 6, 7))
    assert ncc > 0.99 and rot_deg < 1.0 and across < 2.0 and along < 12.0, (ncc, rot_deg, across, along)


@pytest.mark.gpu
def test_training_step_one_volume_per_rank_two_ranks():
    """configs[4] in miniature: every rank renders its own CT, the stand-in regressor's gradients are all-reduced every 4
    steps as one bucket, and the ranks end up with identical weights."""
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", "29541", str(ROOT / "tools" / "train_step_multigpu.py"), "--backend", "gloo", "--single-device",
           "--size", "48", "--det", "32", "--batch", "6", "--steps", "8", "--warmup", "1", "--params", "200000"]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-3000:]
    # (two processes write to one pipe: a report can land behind another line's text instead of on a line of its own)
    import re
    # (so a report ends where the next one starts, or at the end of its line)
    reports = re.findall(r"rank \d/2: .*?(?=rank \d/2: |\n|$)", out.stdout)
    assert len(reports) == 2, out.stdout
    assert all("weights identical across ranks: True" in l and "every 4 steps" in l for l in reports)
