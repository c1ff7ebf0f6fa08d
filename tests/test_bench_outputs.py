"""bench.py's plain line and --dump-outputs: what a plain run prints, and the arrays it leaves for comparing two builds."""
import glob
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_dump_outputs_samples_are_fixed_and_capped(tmp_path):
    """The seeded samples are the same in every run (they are how two builds are compared), integer outputs convert
    exactly, small arrays are written whole, and more than 64 MiB in all is refused."""
    sys.path.insert(0, ROOT)
    import bench
    gen = torch.Generator().manual_seed(0)
    rows = torch.randn(300_000, 3, generator=gen)
    radii = torch.randint(0, 40, (300_000,), generator=gen, dtype=torch.int32)
    plane = torch.randn(1, 4, 300, 300, generator=gen)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), whole={"small": torch.arange(5.0)}, rows={"grad": rows, "radii": radii},
                           elems={"plane": plane}, k_rows=1000, k_elems=500)
    for name, shape in (("small", (5,)), ("grad", (1000, 3)), ("radii", (1000,)), ("plane", (500,))):
        a, b = np.load(tmp_path / "a" / f"{name}.npy"), np.load(tmp_path / "b" / f"{name}.npy")
        assert a.dtype == np.float32 and a.shape == shape and np.array_equal(a, b), name
    idx = bench.seeded_index("grad", rows.shape[0], 1000, "cpu")
    assert np.array_equal(np.load(tmp_path / "a" / "grad.npy"), rows[idx].numpy())
    assert np.array_equal(np.load(tmp_path / "a" / "radii.npy"), radii[bench.seeded_index("radii", 300_000, 1000, "cpu")].numpy())
    with pytest.raises(SystemExit, match="64 MiB"):
        bench.dump_outputs(str(tmp_path / "c"), whole={"big": torch.zeros(17 * 2 ** 20)})
    assert not (tmp_path / "c").exists()


@pytest.mark.gpu
def test_bench_plain_line_and_dump_outputs(tmp_path):
    """`bench.py --gpus 1 --steps K --warmup W --dump-outputs DIR`: one JSON line with the headline fields, exactly K timed
    steps, none of what --full measures, and the last step's image, radii and gradients under DIR in float32, 64 MiB at most."""
    out_dir = tmp_path / "out"
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "2",
           "--dump-outputs", str(out_dir)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    out = json.loads(lines[0])
    assert out["steps"] == 3 and out["warmup"] == 2 and out["ms_per_step"] > 0 and out["value"] > 0
    assert out["unit"] == "Msplats/s" and out["higher_is_better"] is True and out["dtype"] == "f32"
    assert not {"roofline", "kernel_ms", "cfg2", "cpu_baseline", "psnr_match_db", "ramp_ms_per_step"} & set(out)
    files = {os.path.basename(f)[:-4]: np.load(f) for f in glob.glob(str(out_dir / "*.npy"))}
    want = {"image", "radii", "grad_means3D", "grad_opacities", "grad_colors_precomp", "grad_scales", "grad_rotations", "grad_means2D"}
    assert set(files) == want, set(files)
    assert all(a.dtype == np.float32 and np.isfinite(a).all() for a in files.values())
    assert sum(a.nbytes for a in files.values()) <= 64 * 2 ** 20
    assert files["image"].shape == (3, 1080, 1920) and files["radii"].shape == (1 << 18,) and files["grad_means3D"].shape == (1 << 18, 3)
    assert (files["radii"] > 0).any() and np.abs(files["grad_means3D"]).max() > 0
