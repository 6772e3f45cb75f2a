"""bench.py's own launcher: `python bench.py --gpus N` must run N ranks or fail, never report a silent one-rank line.
CPU only: the `--stub` workload exercises the launcher, the rank protocol and the final all_gather over gloo."""
import json
import os
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent


def run(args, env_extra=None, drop=("WORLD_SIZE", "RANK", "LOCAL_RANK")):
    env = {k: v for k, v in os.environ.items() if k not in drop}
    env.update(env_extra or {})
    return subprocess.run([sys.executable, str(ROOT / "bench.py")] + args, capture_output=True, text=True, env=env, timeout=300)


def test_gpus_2_self_launches_two_ranks_gloo():
    r = run(["--gpus", "2", "--stub", "--steps", "3", "--warmup", "1", "--batch", "4"])
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, lines                       # exactly ONE JSON line on stdout
    line = json.loads(lines[0])
    assert line["n_gpus"] == 2 and line["steps"] == 3 and line["warmup"] == 1 and line["data"] == "stub"
    assert line["value"] > 0 and abs(line["value"] - 4 * 2 * 3 / (line["ms_per_step"] * 3e-3)) < 1e-6 * line["value"]


def test_rank_count_mismatch_is_an_error():
    r = run(["--gpus", "2", "--stub"], env_extra={"WORLD_SIZE": "1", "RANK": "0", "LOCAL_RANK": "0"}, drop=())
    assert r.returncode != 0 and "WORLD_SIZE=1" in r.stderr and not r.stdout.strip()


def test_launcher_relays_a_failing_child():
    # no GPU here: the real workload's ranks fail loudly (no CPU fallback) and the launcher returns their non-zero code without a JSON line
    import torch
    if torch.cuda.is_available():
        import pytest
        pytest.skip("needs a GPU-less host")
    r = run(["--gpus", "2", "--steps", "1", "--warmup", "0", "--no-cpu-baseline"])
    assert r.returncode != 0 and not r.stdout.strip()


def test_dump_outputs_same_arguments_same_files(tmp_path):
    # --dump-outputs: the last timed step's output as float32 .npy (here the all-gathered stub rows of both ranks); same arguments, same inputs
    import numpy as np
    for d in ("a", "b"):
        r = run(["--gpus", "2", "--stub", "--steps", "2", "--warmup", "1", "--batch", "3", "--dump-outputs", str(tmp_path / d)])
        assert r.returncode == 0, r.stderr[-2000:]
    a, b = np.load(tmp_path / "a" / "stub_output.npy"), np.load(tmp_path / "b" / "stub_output.npy")
    assert a.dtype == np.float32 and a.shape == (6, 4, 8, 8) and np.array_equal(a, b)
    assert not np.array_equal(a[:3], a[3:])                        # the two ranks' rows (seeded per rank) are both there


def test_dump_outputs_samples_past_the_limit(tmp_path, monkeypatch):
    # past DUMP_LIMIT_BYTES every array keeps the same share of its elements, at seeded positions in index order: the files stay under the
    # limit and two dumps of the same arrays are equal
    import numpy as np
    import torch
    import bench
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 64 << 10)
    arrays = {"x": torch.arange(40000, dtype=torch.float32).reshape(200, 200), "y": torch.ones(1000, dtype=torch.float64), "absent": None}
    for d in ("a", "b"):
        bench.dump_outputs(tmp_path / d, arrays)
    assert sorted(p.name for p in (tmp_path / "a").iterdir()) == ["x.npy", "y.npy"]
    assert sum(p.stat().st_size for p in (tmp_path / "a").iterdir()) <= 64 << 10
    x, y = np.load(tmp_path / "a" / "x.npy"), np.load(tmp_path / "a" / "y.npy")
    assert x.dtype == y.dtype == np.float32 and 0 < x.size < 40000 and 0 < y.size < 1000
    assert np.all(np.diff(x) > 0) and np.all(y == 1)
    assert np.array_equal(x, np.load(tmp_path / "b" / "x.npy"))
    small = {"z": torch.linspace(0, 1, 100)}
    bench.dump_outputs(tmp_path / "c", small)
    assert np.array_equal(np.load(tmp_path / "c" / "z.npy"), small["z"].numpy())
