"""bench.py's command line: a plain run does the timed steps alone, --full
adds the secondary legs, --dump-outputs writes the last step's results."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from jepsen.etcd_amd import abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FULL_ONLY = ("c3_shards", "resident32_leg", "c1_leg", "host_leg", "host_leg32", "host_leg16",
             "search_leg", "mixed_leg", "dropin_leg", "model_leg", "crash_leg", "oversized_key",
             "fanout_leg")


def test_options(monkeypatch):
    import bench
    monkeypatch.setattr(sys, "argv", ["bench.py"])
    a = bench.parse()
    assert not a.full and a.dump_outputs is None
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "d", "--steps", "7"])
    a = bench.parse()
    assert a.full and a.dump_outputs == "d" and a.steps == 7


def test_dump_outputs_writes_every_field(tmp_path):
    import bench
    res = np.zeros(5, dtype=abi.RESULT_DTYPE)
    res["verdict"] = [1, 0, -1, 1, 1]
    res["fail_op"] = [-1, 3, -1, -1, -1]
    res["configs_explored"] = np.arange(5) + (1 << 40)
    d = str(tmp_path / "out")
    bench.dump_outputs(d, res, 0, 1)
    assert sorted(os.listdir(d)) == sorted(f + ".npy" for f in abi.RESULT_DTYPE.names)
    for f in abi.RESULT_DTYPE.names:
        got = np.load(os.path.join(d, f + ".npy"))
        assert got.dtype == np.float64 and got.shape == (5,)
        assert (got == res[f]).all()
    bench.dump_outputs(d, res[:2], 1, 2)
    assert np.load(os.path.join(d, "verdict.rank1.npy")).tolist() == [1.0, 0.0]


def test_dump_outputs_samples_a_large_batch(tmp_path, monkeypatch):
    import bench
    monkeypatch.setattr(bench, "DUMP_MAX_KEYS", 100)
    res = np.zeros(1000, dtype=abi.RESULT_DTYPE)
    res["fail_op"] = np.arange(1000)
    got = []
    for name in ("a", "b"):
        bench.dump_outputs(str(tmp_path / name), res, 0, 1)
        got.append(np.load(str(tmp_path / name / "fail_op.npy")))
    assert got[0].shape == (100,) and (np.diff(got[0]) > 0).all()
    assert (got[0] == got[1]).all()


@pytest.mark.gpu
def test_plain_run_times_the_steps_and_dumps_its_results(ctx, tmp_path):
    """A small plain run: --steps sets the timed steps, the line carries the
    headline fields and none of --full's legs, and the dumped arrays are the
    results lc_check_device gives for the same seeded batch."""
    d = str(tmp_path / "dump")
    out = subprocess.run(
        [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "5",
         "--warmup", "2", "--keys", "300", "--ops-per-key", "100", "--dump-outputs", d],
        stdout=subprocess.PIPE, timeout=120, check=True).stdout.decode()
    lines = out.strip().splitlines()
    assert len(lines) == 1
    line = json.loads(lines[0])
    assert line["steps"] == 5 and line["warmup"] == 2 and line["n_gpus"] == 1
    assert line["unit"] == "ops/s" and line["higher_is_better"] is True
    assert line["dtype"] == "int32" and line["metric"]
    assert line["ms_per_step"] > 0
    assert line["value"] == pytest.approx(300 * 100 / (line["ms_per_step"] * 1e-3), rel=1e-6)
    assert line["verdicts"] == {"valid": 300, "invalid": 0, "unknown": 0}
    assert line["cpu_baseline"] is None and line["hot_key"] is None
    assert not [k for k in FULL_ONLY if k in line]
    ops, off, _, _ = abi.synth(300, 100, concurrency=20, p_info=0.0, seed=0x5EED0002)
    import torch
    dev = torch.device("cuda", 0)
    d_ops, d_off = torch.from_numpy(ops).to(dev), torch.from_numpy(off).to(dev)
    d_out = torch.zeros(300 * abi.RESULT_DTYPE.itemsize, dtype=torch.uint8, device=dev)
    ctx.check_device(d_ops.data_ptr(), d_off.data_ptr(), 300, d_out.data_ptr(),
                     stream=torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize()
    want = np.frombuffer(d_out.cpu().numpy().tobytes(), dtype=abi.RESULT_DTYPE)
    for f in abi.RESULT_DTYPE.names:
        got = np.load(os.path.join(d, f + ".npy"))
        assert got.dtype == np.float64 and (got == want[f]).all(), f
