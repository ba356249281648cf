"""A plain bench.py run end to end on a tiny scene (8 views of 32x32, 256 rays x 64 samples):
the step counts, the result line of a plain run and the --dump-outputs files."""

import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PLAIN_KEYS = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps",
              "warmup", "final_loss", "nonfinite_params")
FULL_ONLY = ("windows", "transient_window", "roofline", "roofline_targets", "cpu_baseline",
             "strong_scaling", "alt_numerics", "peaks", "kernels", "kernels_source")


@pytest.mark.gpu
def test_plain_run_steps_line_and_dump(dev, tmp_path, monkeypatch, capsys):
    sys.path.insert(0, ROOT)
    import bench

    calls = {"step": 0}
    real_step = bench.IngpJob.step

    def counting_step(self):
        calls["step"] += 1
        return real_step(self)

    monkeypatch.setattr(bench.IngpJob, "step", counting_step)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    out = tmp_path / "dump"
    steps, warmup, settle, batch = 3, 1, 4, 256
    monkeypatch.setattr(sys, "argv", [
        "bench.py", "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup), "--views", "8",
        "--img-size", "32", "--batch", str(batch), "--samples", "64", "--settle", str(settle),
        "--graph", "off", "--dump-outputs", str(out)])
    import torch

    rng = torch.get_rng_state(), torch.cuda.get_rng_state(dev)
    try:
        bench.main()
    finally:  # the benchmark seeds the generators; later tests keep the stream they had
        torch.set_rng_state(rng[0])
        torch.cuda.set_rng_state(rng[1], dev)
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.strip()]
    assert len(lines) == 1  # the JSON line is the only stdout line
    line = json.loads(lines[0])

    # step() runs for the warm start (10 build-numerics steps), the settle, the warm-up and
    # the timed steps, and for nothing else in a plain run
    assert calls["step"] == 10 + settle + warmup + steps
    for k in PLAIN_KEYS:
        assert k in line, k
    for k in FULL_ONLY:
        assert k not in line, k
    assert (line["steps"], line["warmup"], line["full"]) == (steps, warmup, False)
    assert line["metric"] == "train-step rays/sec" and line["unit"] == "rays/s"
    assert line["higher_is_better"] is True and line["dtype"] == "f16"
    assert line["nonfinite_params"] == 0
    # value and ms_per_step describe the same timed region (ms_per_step is rounded to 1 us)
    assert line["value"] * line["ms_per_step"] * 1e-3 == pytest.approx(batch, rel=0.02)

    def load(d):
        arrs = {f[:-4]: np.load(os.path.join(d, f)) for f in os.listdir(d) if f.endswith(".npy")}
        for name, a in arrs.items():
            assert a.dtype == np.float32 and np.isfinite(a).all(), name
        return arrs

    probe, last = load(out), load(out / "last_step")
    maps = {"color_map_fine", "color_map_atmo", "color_map_surf", "color_surf"}
    assert set(last) == {"loss"} | maps
    assert set(probe) == ({"loss", "sigma_fine", "color_fine"} | maps
                          | {"step2_" + k for k in {"loss"} | maps}
                          | {"grad_" + m for m in ("pos_encoder", "pos_mlp", "dir_mlp",
                                                   "surf_encoder", "surf_mlp")})
    assert sum(a.nbytes for a in {**probe, **{"l_" + k: v for k, v in last.items()}}.values()) \
        < 64e6
    assert last["loss"].item() == pytest.approx(line["final_loss"], abs=1e-6)
    assert last["color_map_fine"].shape == (batch * 4,)
    assert probe["sigma_fine"].shape == (batch * 63,)
    # the surface branch sets the initial colour maps, so its gradients cannot vanish; the
    # field's may (reference numerics: with the initial weights ~1e-5 the f16 composite
    # underflows dL/dcolor), so nothing is asked of them here
    for name in ("grad_surf_encoder", "grad_surf_mlp"):
        assert np.count_nonzero(probe[name]) > 0, name
