"""bench.py's plain run and --dump-outputs: the frame the last timed step delivered, written as float32 .npy within the size
limit (a seeded sample of the pixels beyond it), and a plain line that carries the headline without the --full side figures."""
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    spec = importlib.util.spec_from_file_location("bench_for_test", os.path.join(ROOT, "bench.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_dump_unpacks_the_packed_framebuffer(tmp_path):
    px = np.random.default_rng(7).integers(0, 1 << 24, (48, 64)).astype(np.int32)
    _bench().dump_frame(str(tmp_path), px)
    f = np.load(tmp_path / "frame.npy")
    assert f.dtype == np.float32 and f.shape == (48, 64, 3) and not (tmp_path / "frame_index.npy").exists()
    back = (f[..., 0].astype(np.int64) << 16) | (f[..., 1].astype(np.int64) << 8) | f[..., 2].astype(np.int64)
    assert np.array_equal(back, px)


def test_dump_of_a_large_frame_is_a_fixed_sample_within_the_limit(tmp_path, monkeypatch):
    m = _bench()
    monkeypatch.setattr(m, "DUMP_LIMIT", 200_000)
    frame = np.random.default_rng(3).random((120, 160, 5), dtype=np.float32)  # 384 kB
    for d in ("a", "b"):
        m.dump_frame(str(tmp_path / d), frame)
    sizes = sum(os.path.getsize(tmp_path / "a" / n) for n in ("frame.npy", "frame_index.npy"))
    assert sizes <= 200_000
    idx, s = np.load(tmp_path / "a" / "frame_index.npy"), np.load(tmp_path / "a" / "frame.npy")
    assert idx.dtype == np.float64 and s.dtype == np.float32 and s.shape == (len(idx), 5) and np.all(np.diff(idx) > 0)
    assert np.array_equal(s, frame.reshape(-1, 5)[idx.astype(np.int64)])
    assert np.array_equal(idx, np.load(tmp_path / "b" / "frame_index.npy"))  # the same sample every run


@pytest.mark.gpu
def test_plain_run_times_the_steps_and_dumps_the_last_frame(built, tmp_path):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--scene", "S2", "--steps", "7", "--warmup", "2",
                        "--dump-outputs", str(tmp_path)], capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, (r.stdout[-800:], r.stderr[-2500:])
    line = json.loads([ln for ln in r.stdout.strip().splitlines() if ln.startswith("{")][-1])
    assert line["steps"] == 7 and line["ms_per_step"] > 0 and line["value"] > 0 and line["full"] is False
    assert line["roofline"] is None and line["latency"] is None and line["cpu_baseline"] is None and line["fixed_camera"] is None
    f = np.load(tmp_path / "frame.npy")
    assert f.dtype == np.float32 and f.shape == (line["config"]["height"], line["config"]["width"], 3)
    assert f.min() >= 0 and f.max() <= 255 and f.max() > 0 and np.array_equal(f, np.round(f))
