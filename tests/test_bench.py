"""bench.py: a plain run prints the headline line without the --full legs, and --dump-outputs writes what its last timed
step computed - the frame the library renders for the same configuration - within the size limit."""
import json
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import bench  # noqa: E402


def test_dump_outputs_takes_a_fixed_sample_of_a_large_array(tmp_path, monkeypatch):
    import torch
    monkeypatch.setattr(bench, "DUMP_BYTES", 1 << 16)
    small = torch.arange(30, dtype=torch.uint8).view(-1, 3)
    big = torch.rand(100000, 3, generator=torch.Generator().manual_seed(1))
    for d in ("a", "b"):
        bench.dump_outputs(tmp_path / d, {"rgb8": small, "accum": big})
    assert sorted(p.name for p in (tmp_path / "a").iterdir()) == ["accum.npy", "accum_rows.npy", "rgb8.npy"]
    assert sum(p.stat().st_size for p in (tmp_path / "a").iterdir()) <= (1 << 16) + 3 * 128   # (+ the .npy headers)
    rgb = np.load(tmp_path / "a" / "rgb8.npy")
    assert rgb.dtype == np.float32 and np.array_equal(rgb, small.numpy())
    acc, rows = np.load(tmp_path / "a" / "accum.npy"), np.load(tmp_path / "a" / "accum_rows.npy")
    assert acc.dtype == np.float32 and rows.dtype == np.float64 and len(rows) > 1000
    assert np.all(np.diff(rows) > 0) and np.array_equal(acc, big.numpy()[rows.astype(np.int64)])
    assert np.array_equal(rows, np.load(tmp_path / "b" / "accum_rows.npy"))   # the same rows every run


@pytest.mark.gpu
def test_plain_run_dumps_the_frame_the_library_renders(tmp_path, pta):
    w, h, spp, bounces, tris = 96, 64, 4, 3, 3000
    cmd = [sys.executable, str(ROOT / "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1", "--tris", str(tris),
           "--width", str(w), "--height", str(h), "--spp", str(spp), "--bounces", str(bounces),
           "--dump-outputs", str(tmp_path / "out")]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert line["steps"] == 2 and line["value"] > 0 and line["ms_per_step"] > 0
    assert line["unit"] == "Msamples/s" and line["higher_is_better"] is True and line["dtype"] == "f32"
    assert line["roofline"] is None and line["cpu_baseline"] is None and line["config"]["legacy_framing"] is None
    g = pta.GpuScene(pta.HostScene.generate_ps5(tris, 0, 8), device=0)
    rgb, acc = g.render(pta.Profile.make(w, h, spp, bounces, "FILMIC"))
    assert sorted(p.name for p in (tmp_path / "out").iterdir()) == ["accum.npy", "rgb8.npy"]
    d_rgb, d_acc = np.load(tmp_path / "out" / "rgb8.npy"), np.load(tmp_path / "out" / "accum.npy")
    assert d_rgb.dtype == np.float32 and d_acc.dtype == np.float32
    assert np.array_equal(d_rgb, rgb.astype(np.float32))
    assert np.array_equal(d_acc.view(np.uint32), acc.view(np.uint32))
