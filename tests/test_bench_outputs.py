"""bench.py --dump-outputs: the arrays the last timed step left (lde, leaves, nodes, cap) as
float64 (high, low) 32-bit halves of the canonical values, large arrays as a fixed seeded sample
of flat positions; and the plain run's line, which carries the headline and none of --full's legs."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = (1 << 64) - (1 << 32) + 1


def _join(a):
    """(..., 2) float64 halves -> uint64."""
    assert a.dtype == np.float64 and a.shape[-1] == 2
    return (a[..., 0].astype(np.uint64) << np.uint64(32)) | a[..., 1].astype(np.uint64)


def test_dump_array_is_exact_and_canonical():
    import torch
    import bench
    v = np.array([[0, 1, P - 1, P, P + 5, (1 << 64) - 1], [1 << 32, (1 << 32) - 1, 1 << 63, 12345, P - 2, 7]],
                 dtype=np.uint64)
    a = bench.dump_array(torch.from_numpy(v.view(np.int64)), 1)
    assert a.shape == (2, 6, 2)
    assert _join(a).tolist() == [[int(x) % P for x in row] for row in v]


def test_dump_array_samples_the_same_positions_every_time(monkeypatch):
    import torch
    import bench
    monkeypatch.setattr(bench, "DUMP_MAX_ELEMS", 1000)
    v = np.random.RandomState(3).randint(0, 1 << 62, size=(7, 11, 101), dtype=np.int64)
    t = torch.from_numpy(v)
    a, b = bench.dump_array(t, 5), bench.dump_array(t, 5)
    assert a.shape == (1000, 2) and np.array_equal(a, b)
    idx = np.sort(np.random.RandomState(5).randint(0, v.size, size=1000, dtype=np.int64))
    assert np.array_equal(_join(a), v.reshape(-1)[idx].astype(np.uint64))
    # at the limit the whole array is kept, in its own shape
    assert bench.dump_array(t.reshape(-1)[:1000].reshape(10, 100), 5).shape == (10, 100, 2)


def test_steps_must_be_positive():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0"], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 2 and "--steps" in r.stderr


@pytest.mark.gpu
def test_plain_run_dumps_the_commit(tmp_path):
    """One plain C1 run (2^16 x 32, LDE x2): the line has the headline fields and no --full leg, and
    the dumped arrays are the oracle's commit of the same synthetic trace (lde at the sampled
    positions; leaves, nodes and cap whole)."""
    import bench
    import oracle
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--config", "C1", "--steps", "3",
                        "--warmup", "1", "--dump-outputs", str(tmp_path)], env=env, capture_output=True, text=True,
                       timeout=240)
    assert r.returncode == 0, r.stderr
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    line = json.loads(lines[0])
    assert line["steps"] == 3 and line["warmup"] == 1 and line["full"] is False
    assert line["unit"] == "elems/s" and line["higher_is_better"] is True and line["dtype"] == "u64 (Goldilocks)"
    assert line["ms_per_step"] > 0
    assert abs(line["value"] - 32 * (1 << 16) / (line["ms_per_step"] * 1e-3)) <= 1e-9 * line["value"]
    assert set(line["phase_ms"]) == {"lde", "leaves", "nodes"}
    for k in ("verified", "roofline", "roofline_ntt", "cpu_baseline", "native_ms_per_step"):
        assert k not in line

    n_cols, log_n, log_lde, cap = bench.CONFIGS["C1"]
    ref = oracle.lde_commit(oracle.synthetic_trace(n_cols, log_n), log_lde, cap, threads=4)
    assert sorted(os.listdir(tmp_path)) == ["cap.npy", "lde.npy", "leaves.npy", "nodes.npy"]
    assert sum(os.path.getsize(tmp_path / f) for f in os.listdir(tmp_path)) <= 64 * 10 ** 6
    for name in ("leaves", "nodes", "cap"):
        assert np.array_equal(_join(np.load(tmp_path / (name + ".npy"))), ref[name] % np.uint64(P)), name
    flat = ref["lde"].reshape(-1)
    assert flat.size > bench.DUMP_MAX_ELEMS
    idx = np.sort(np.random.RandomState(bench.DUMP_SEED).randint(0, flat.size, size=bench.DUMP_MAX_ELEMS,
                                                                 dtype=np.int64))
    assert np.array_equal(_join(np.load(tmp_path / "lde.npy")), flat[idx] % np.uint64(P))
