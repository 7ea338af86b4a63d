"""bench.py's command line: a plain run does the C2 steps alone, --full keeps every other measurement, and
--dump-outputs writes the last timed step's statuses as .npy (bounded in size, a fixed sample beyond the bound)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import bench

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXTRAS = ("tagg_groups", "cpu_sample", "rlc_node_validators", "latency_calls", "c5", "keys", "host_path")


def _parse(monkeypatch, *argv):
    monkeypatch.setattr(sys, "argv", ["bench.py"] + list(argv))
    return bench.parse()


def test_plain_run_switches_every_extra_off(monkeypatch):
    a = _parse(monkeypatch, "--gpus", "1", "--steps", "7", "--warmup", "2", "--tagg-groups", "50")
    assert (a.steps, a.warmup, a.full, a.dump_outputs) == (7, 2, False, None)
    assert [getattr(a, k) for k in EXTRAS] == [0] * len(EXTRAS)
    assert a.n == 65536  # the headline workload is untouched


def test_full_keeps_the_extras_and_their_sizes(monkeypatch):
    a = _parse(monkeypatch, "--full", "--tagg-groups", "50", "--dump-outputs", "d")
    assert a.full and a.dump_outputs == "d" and a.tagg_groups == 50
    assert all(getattr(a, k) > 0 for k in EXTRAS)


def test_dump_outputs_writes_float32_and_samples_past_the_bound(tmp_path, monkeypatch):
    st = np.array([0, 3, 2, 0, 1], dtype=np.int32)
    bench.dump_outputs(str(tmp_path / "a"), {"verify_status": st.tolist(), "node_bitmap": st == 0})
    got = np.load(tmp_path / "a" / "verify_status.npy")
    assert got.dtype == np.float32 and got.tolist() == st.tolist()
    assert np.load(tmp_path / "a" / "node_bitmap.npy").tolist() == [1, 0, 0, 1, 0]
    # past the bound: the same sorted sample of positions on every call, the files within the bound
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 4096)
    big = np.arange(5000)
    for d in ("b", "c"):
        bench.dump_outputs(str(tmp_path / d), {"x": big, "y": big % 7})
    x, y = np.load(tmp_path / "b" / "x.npy"), np.load(tmp_path / "b" / "y.npy")
    assert 0 < x.size < 5000 and np.all(np.diff(x) > 0) and np.array_equal(y, x % 7)
    assert np.array_equal(x, np.load(tmp_path / "c" / "x.npy"))
    assert sum(os.path.getsize(tmp_path / "b" / f) for f in os.listdir(tmp_path / "b")) <= 4096


@pytest.mark.gpu
def test_plain_run_dumps_the_statuses_of_the_seeded_batch(tmp_path):
    """The benchmark itself, small: one plain run, its line and its dumped statuses against the batch's construction."""
    n = 512
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
                        "--c2-items", str(n), "--dump-outputs", str(tmp_path)],
                       capture_output=True, text=True, timeout=120, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr[-2000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert line["steps"] == 2 and line["full"] is False and line["ms_per_step"] > 0
    assert line["value"] == pytest.approx(n / (line["ms_per_step"] * 1e-3), rel=1e-2)
    for k in ("threshold_aggregates_per_s", "drop_in_latency", "host_path"):
        assert line[k] is None
    assert "rlc_batch_verify" not in line and "cpu_baseline" not in line and "full_slot_mix" not in line
    st = np.load(tmp_path / "verify_status.npy")
    assert st.dtype == np.float32 and st.shape == (n,)
    assert {i for i in range(n) if st[i] != 0} == {i for i in range(n) if bench.c2_is_bad(i)[0]}
    assert os.listdir(tmp_path) == ["verify_status.npy"]
