"""bench.py's plain run (no --full) and --dump-outputs.

A plain run carries the headline fields and none of the secondary measurements; the
frames it dumps are the last timed step's, named by their animation frame, and each is
the oracle's frame of that scene bit for bit -- whole at config 1 (256 x 256), a seeded
pixel sample at config 2 (1920 x 1080), where four frames exceed the dump's budget."""
import glob
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import bits_equal, first_mismatch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NT = min(16, os.cpu_count() or 1)


def _bench():
    sys.path.insert(0, ROOT)
    import bench
    return bench


def test_dump_outputs_picks_and_sample(tmp_path):
    """dump_outputs on host tensors: the frames still in the ring after the last step,
    evenly spaced with the last one among them; whole frames under the budget, else one
    seeded sample of pixels, the same for every frame and every call."""
    import torch
    bench = _bench()
    # 6 timed frames in steps of 3 over a ring of 4: frames 3, 4, 5 are the last step's
    W, H = 8, 4
    ring = [torch.full((H, W, 4), float(s), dtype=torch.float32) for s in range(4)]
    d = bench.dump_outputs(str(tmp_path / "a"), ring, lambda i: i % 4, 6, 3, lambda i: 100 + i, W, H)
    assert d["arrays"] == ["frame_000103", "frame_000104", "frame_000105"] and d["sample"] is None
    for name, slot in zip(d["arrays"], (3, 0, 1)):
        a = np.load(tmp_path / "a" / (name + ".npy"))
        assert a.dtype == np.float32 and a.shape == (H, W, 4) and (a == slot).all()
    # frames over the budget: the same sorted sample of pixel indices of each
    W, H = 2048, 1024
    base = torch.arange(W * H, dtype=torch.float32).view(H, W, 1).expand(H, W, 4).contiguous()
    ring = [base + k for k in range(2)]
    for run in ("b", "c"):
        d = bench.dump_outputs(str(tmp_path / run), ring, lambda i: i % 2, 8, 2, lambda i: i, W, H)
    assert d["arrays"] == ["frame_000006", "frame_000007"]
    n = bench.DUMP_BYTES // (16 * 2)
    assert d["pixels_per_frame"] == n < W * H
    a6, a7 = (np.load(tmp_path / "b" / f"frame_00000{k}.npy") for k in (6, 7))
    assert a6.shape == (n, 4) and a6.dtype == np.float32
    idx = a6[:, 0].astype(np.int64)
    assert (np.diff(idx) > 0).all() and idx[0] >= 0 and idx[-1] < W * H
    assert np.array_equal(a7, a6 + 1)
    assert np.array_equal(a6, np.load(tmp_path / "c" / "frame_000006.npy"))
    assert sum(os.path.getsize(f) for f in glob.glob(str(tmp_path / "b" / "*.npy"))) <= 64 << 20


@pytest.mark.gpu
@pytest.mark.parametrize("config", [1, 2])
def test_plain_run_dumps_the_last_steps_frames(config, tmp_path, oracle, scenes):
    bench = _bench()
    steps, warmup, fps = 2, 1, 8
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps),
                        "--warmup", str(warmup), "--config", str(config), "--frames-per-step", str(fps),
                        "--preroll-ms", "0", "--dump-outputs", str(tmp_path)],
                       capture_output=True, text=True, timeout=120, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout
    res = json.loads(lines[0])
    cfg = scenes.CONFIGS[config]
    W, H, K = cfg["width"], cfg["height"], cfg["steps"]
    # the headline fields, and nothing that needs a pass of its own
    assert res["full"] is False and res["steps"] == steps and res["frames_per_step"] == fps
    assert res["unit"] == "Mpixels/s" and res["higher_is_better"] is True and res["dtype"] == "f64"
    assert res["value"] == pytest.approx(fps * W * H / (res["ms_per_step"] * 1e-3) / 1e6, rel=1e-2)
    for k in ("roofline", "roofline_other_kernel", "roofline_frame", "one_lane", "alt_fused_shadow", "tile_gather",
              "host_output"):
        assert res[k] is None, k
    assert "cpu_baseline" not in res
    # the last step's frames: timed frames 8..15 are animation frames 16..23 (after 8 warmup frames)
    d = res["dumped_outputs"]
    first, last = (warmup + steps - 1) * fps, (warmup + steps) * fps - 1
    assert d["arrays"] == [f"frame_{i:06d}" for i in range(first + 1, last + 1, 2)]
    assert sorted(os.path.basename(f) for f in glob.glob(str(tmp_path / "*.npy"))) == [n + ".npy" for n in d["arrays"]]
    idx = None
    if config == 2:
        n = bench.DUMP_BYTES // (16 * len(d["arrays"]))
        assert d["pixels_per_frame"] == n < W * H
        idx = np.sort(np.random.default_rng(bench.DUMP_SEED).choice(W * H, size=n, replace=False))
    eye, sh = scenes.eye_camera(), scenes.shadow_camera()
    total = 0
    for name in d["arrays"]:
        got = np.load(tmp_path / (name + ".npy"))
        total += got.nbytes
        i = int(name.split("_")[1])
        scene = scenes.closely_orbiting_sphere(100 + i) if config == 1 else scenes.scene_a_bench(100 + i)
        want = oracle.render(scene, eye, sh, W, H, K, cfg["flags"], nthreads=NT)["rgba"]
        if idx is not None:
            want = np.ascontiguousarray(want.reshape(W * H, 4)[idx])
        assert got.dtype == np.float32
        assert bits_equal(got, want), (name, first_mismatch(got, want))
    assert total <= 64 << 20
