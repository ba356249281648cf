"""What multi_band_extinction costs, on one commit and in one process.

At 8,192 rays x 1,024 samples (the bench shape), timed with device events after warm-up,
the arms of each group alternating:

* the Instant-NGP train step (forward, loss, backward, AdamW) with ``multi_band_extinction``
  and four bands, ``fused=True`` (the fused field kernels with S = 4 density outputs)
  against ``fused=False`` (op by op through the module kernels), and the one-band fused
  step beside them;
* anr_ingp_field_fwd and anr_ingp_field_bwd alone through the C ABI, S = 4 (a dir network
  of 16 inputs, sigma / d_sigma (M, 4)) against S = 1 (19 inputs, (M,)), W = 64, two dir
  hidden layers, f16, level-quad planes: the sigma and d_sigma streams grow by 12 B per
  sample each way, everything else is the same traffic.

    python tools/multiband_timing.py [--rays 8192] [--samples 1024] [--reps 10]

Prints one JSON line; times are milliseconds per call (median and minimum over --reps).
"""

from __future__ import annotations

import argparse
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "atmospheric-neural-rendering_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

import __graft_entry__ as ge  # noqa: E402
from atmonr_amd import _lib  # noqa: E402

OPT = {"lr": 1e-2, "betas": [0.9, 0.99], "eps": 1e-15, "weight_decay": 1e-2}


def _time(fns: dict, reps: int, warm: int = 3) -> dict:
    """Each callable ``reps`` times, alternating between them; ms per call."""
    for fn in fns.values():  # warm-up: code objects, allocator
        for _ in range(warm):
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ms[k].append(a.elapsed_time(b))
    return {k: {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4)}
            for k, v in ms.items()}


def _field_kernels(dev, M: int, n_per_ray: int, reps: int) -> dict:
    lib = _lib.load()
    s = _lib.stream(dev)
    gen = torch.Generator(device=dev).manual_seed(7)
    width, nhd, nb = 64, 2, 4
    planes = (torch.rand(4, M, 8, device=dev, generator=gen) * 2 - 1).half()
    dirs = torch.rand(M // n_per_ray, 3, device=dev, generator=gen)
    dcol = torch.randn(M, nb, device=dev, generator=gen) * 1e-2
    d_enc = torch.empty(M, 32, device=dev)
    color = torch.empty(M, nb, device=dev)
    fwd, bwd, keep = {}, {}, []
    for S in (1, 4):
        pdsc = _lib.mlp_desc(32, 16, width, 1, False)
        ddsc = _lib.mlp_desc(20 - S, nb, width, nhd, False)
        pb, db = ctypes.byref(pdsc), ctypes.byref(ddsc)
        pp = torch.randn(lib.anr_mlp_n_params(pb), device=dev, generator=gen) * (2.0 / 32) ** 0.5
        pd = torch.randn(lib.anr_mlp_n_params(db), device=dev, generator=gen) * (2.0 / width) ** 0.5
        packed = torch.empty(lib.anr_ingp_field_packed_size(pb, db), device=dev,
                             dtype=torch.float16)
        _lib.call("anr_ingp_field_pack", pb, db, _lib.F16, pp.data_ptr(), pd.data_ptr(),
                  packed.data_ptr(), s)
        sigma = torch.empty(M, S, device=dev)
        dsig = torch.randn(M, S, device=dev, generator=gen) * 1e-3
        g_pos, g_dir = torch.zeros_like(pp), torch.zeros_like(pd)
        ws_bytes = lib.anr_ingp_field_bwd_workspace_bytes(pb, db, _lib.F16, M)
        ws = torch.empty(max(1, ws_bytes // 4), device=dev)
        keep += [pdsc, ddsc, pp, pd, packed, sigma, dsig, g_pos, g_dir, ws]

        def f(pb=pb, db=db, packed=packed, sigma=sigma):
            _lib.call("anr_ingp_field_fwd", pb, db, _lib.F16, packed.data_ptr(),
                      planes.data_ptr(), -8 * M, dirs.data_ptr(), n_per_ray, M, sigma.data_ptr(),
                      color.data_ptr(), nb, s)

        def b(pb=pb, db=db, packed=packed, dsig=dsig, g_pos=g_pos, g_dir=g_dir, ws=ws,
              ws_bytes=ws_bytes):
            _lib.call("anr_ingp_field_bwd", pb, db, _lib.F16, packed.data_ptr(),
                      planes.data_ptr(), -8 * M, dirs.data_ptr(), n_per_ray, M, dsig.data_ptr(),
                      dcol.data_ptr(), nb, d_enc.data_ptr(), 32, g_pos.data_ptr(),
                      g_dir.data_ptr(), ws.data_ptr(), ws_bytes, s)

        fwd[f"S{S}"], bwd[f"S{S}"] = f, b
    out = {"field_fwd_f16": _time(fwd, reps), "field_bwd_f16": _time(bwd, reps)}
    del keep
    return out


def _train_steps(dev, B: int, N: int, reps: int) -> dict:
    from atmonr_amd.datasets.synthetic import SyntheticHARP2Dataset
    from atmonr_amd.pipelines.instant_ngp import InstantNGPPipeline

    ds = SyntheticHARP2Dataset(n_views=8, img_size=32, device=dev, seed=0)
    gen = torch.Generator(device=dev).manual_seed(7)
    idx = torch.randint(0, len(ds), (B,), device=dev, generator=gen)
    batch = ds.__getbatch__(idx)
    steps = {}
    for name, multi, fused in (("multiband_fused", True, True),
                               ("multiband_unfused", True, False),
                               ("one_band_fused", False, True)):
        cfg = ge._ingp_config(N)
        cfg.update(multi_band_extinction=multi)
        pipe = InstantNGPPipeline(cfg, ds, fused=fused)
        pipe.send_tensors_to(dev)
        assert pipe.fused is fused, name
        opt = pipe.get_optimizer(OPT)

        def step(pipe=pipe, opt=opt):
            loss = pipe.compute_loss(batch, pipe.forward(batch))
            opt.zero_grad()
            loss.backward()
            opt.step()

        steps[name] = step
    out = _time(steps, reps)
    out["fused_over_unfused"] = round(out["multiband_fused"]["median_ms"] /
                                      out["multiband_unfused"]["median_ms"], 4)
    return out


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rays", type=int, default=8192)
    ap.add_argument("--samples", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=10)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("multiband_timing: no GPU (times are measured on the device only)")
    dev = torch.device("cuda:0")
    out = {"rays": a.rays, "samples": a.samples}
    out.update(_field_kernels(dev, a.rays * a.samples, a.samples, a.reps))
    torch.cuda.empty_cache()
    out["train_step"] = _train_steps(dev, a.rays, a.samples, a.reps)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
