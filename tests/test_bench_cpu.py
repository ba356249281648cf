"""bench.py's launch contract on CPU (no GPU call is made): `--gpus N` without a
torch.distributed environment starts N ranks through torch.distributed.run on 127.0.0.1
in a child process, and a WORLD_SIZE that disagrees with --gpus fails loudly."""

import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_gpus_n_launches_n_ranks(monkeypatch):
    sys.path.insert(0, ROOT)
    import bench

    seen = {}

    def fake_call(cmd, env=None):
        seen["cmd"], seen["env"] = cmd, env
        return 7

    monkeypatch.setattr(subprocess, "call", fake_call)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "4", "--steps", "3"])
    try:
        bench.main()
    except SystemExit as e:
        assert e.code == 7  # the ranks' exit status is passed through
    else:
        raise AssertionError("bench.main() returned without exiting")
    cmd = seen["cmd"]
    assert cmd[1:3] == ["-m", "torch.distributed.run"]
    assert "--nproc-per-node=4" in cmd and "127.0.0.1" in cmd
    assert cmd[-4:] == ["--gpus", "4", "--steps", "3"]
    assert seen["env"]["HSA_ENABLE_IPC_MODE_LEGACY"] == "0"


def test_dump_outputs_float_arrays_and_fixed_sample(tmp_path):
    """--dump-outputs files: float32 (float64 kept), whole when small, and for a large
    output the same seeded sample of DUMP_SAMPLE elements in every call."""
    import numpy as np
    import torch

    sys.path.insert(0, ROOT)
    import bench

    big = torch.arange(bench.DUMP_SAMPLE * 3, dtype=torch.float32)
    arrays = {"loss": torch.tensor(0.5, dtype=torch.float16),
              "small": torch.arange(12, dtype=torch.float64).view(3, 4), "big": big}
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    bench.dump_outputs(a, arrays)
    bench.dump_outputs(b, arrays)
    assert sorted(os.listdir(a)) == ["big.npy", "loss.npy", "small.npy"]
    loss, small, s = (np.load(os.path.join(a, f"{n}.npy")) for n in ("loss", "small", "big"))
    assert loss.dtype == np.float32 and loss.tolist() == [0.5]
    assert small.dtype == np.float64 and small.tolist() == list(range(12))
    assert s.dtype == np.float32 and s.shape == (bench.DUMP_SAMPLE,)
    assert np.all(np.diff(s) >= 0) and s.min() >= 0 and s.max() < big.numel()
    assert s.max() - s.min() > 2.9 * bench.DUMP_SAMPLE  # drawn over the whole array
    assert np.array_equal(s, np.load(os.path.join(b, "big.npy")))
    # what is dumped of a step: the loss and the per-ray maps of its forward, nothing else
    res = {"color_map_fine": big[:8], "sigma_fine": big, "color_surf": big[:4]}
    assert sorted(bench.step_outputs(arrays["loss"], res)) == ["color_map_fine", "color_surf",
                                                               "loss"]
    assert list(bench.step_outputs(arrays["loss"])) == ["loss"]


def test_world_size_mismatch_fails():
    env = dict(os.environ, WORLD_SIZE="2", RANK="0", LOCAL_RANK="0")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "4"],
                       env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "WORLD_SIZE=2" in r.stderr
