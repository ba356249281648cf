"""What the fourth dimension costs (include_height), on one commit and in one process.

At 8,192 rays x 1,024 ray-like samples with the config-3 grid (16 levels, base 16, scale
1.3819, T = 2^19), timed with device events after warm-up, 3-D and 4-D alternating:

* anr_hashgrid_fwd_planes, f16 table (16 corner gathers per level in 4-D, 8 in 3-D);
* anr_hashgrid_bwd, f32 gradients (4-D runs the v1 walker, 3-D the v2 walker);
* the fused sampler with the horizontal preprocessor (mode 1), with the raw points
  (mode 0) and with the height appended (mode 2).

    python tools/hashgrid4d_timing.py [--rays 8192] [--samples 1024] [--reps 10]

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

from atmonr_amd import _lib  # noqa: E402
from atmonr_amd.samplers import sample_and_preprocess  # noqa: E402


def _time(fns: dict, reps: int) -> dict:
    """Each callable ``reps`` times, alternating between them; ms per call."""
    for fn in fns.values():  # warm-up: code objects, allocator
        for _ in range(3):
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


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rays", type=int, default=8192)
    ap.add_argument("--samples", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=10)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("hashgrid4d_timing: no GPU (times are measured on the device only)")
    dev = torch.device("cuda:0")
    s = _lib.stream(dev)
    B, N = a.rays, a.samples
    M = B * N
    gen = torch.Generator(device=dev).manual_seed(7)
    o = torch.rand(B, 1, 4, device=dev, generator=gen)
    dr = (torch.rand(B, 1, 4, device=dev, generator=gen) - 0.5) * 0.6
    t = torch.linspace(0, 1, N, device=dev)[None, :, None]
    x4 = (o + dr * t).clamp(0, 1)
    x4[..., 3] = x4[..., 3] * 2.0 - 0.5  # a height leaves [0, 1]
    x4 = x4.reshape(M, 4).contiguous()
    x3 = x4[:, :3].contiguous()
    out = {"rays": B, "samples": N}

    fwd, bwd = {}, {}
    keep = []
    for D, x in ((3, x3), (4, x4)):
        d = _lib.hashgrid_desc(D, 16, 2, 16, 1.3819, 19, allow_4d=True)
        table = ((torch.rand(d.n_params, device=dev, generator=gen) * 2 - 1) * 1e-2).half()
        planes = torch.empty(4, M, 8, device=dev, dtype=torch.float16)
        g = torch.randn(M, 32, device=dev, generator=gen)
        dtab = torch.zeros(d.n_params, device=dev)
        keep += [d, table, planes, g, dtab]

        def f(d=d, x=x, D=D, table=table, planes=planes):
            _lib.call("anr_hashgrid_fwd_planes", ctypes.byref(d), x.data_ptr(), D, M,
                      table.data_ptr(), _lib.F16, planes.data_ptr(), 8 * M, s)

        def b(d=d, x=x, D=D, g=g, dtab=dtab):
            _lib.call("anr_hashgrid_bwd", ctypes.byref(d), x.data_ptr(), D, M, g.data_ptr(),
                      _lib.F32, 32, dtab.data_ptr(), s)

        fwd[f"{D}d"], bwd[f"{D}d"] = f, b
    out["hashgrid_fwd_planes_f16"] = _time(fwd, a.reps)
    out["hashgrid_bwd_f32"] = _time(bwd, a.reps)
    del keep, fwd, bwd

    from atmonr_amd.datasets.synthetic import SyntheticHARP2Dataset

    ds = SyntheticHARP2Dataset(n_views=8, img_size=32, device=dev, seed=0)
    idx = torch.randint(0, len(ds), (B,), device=dev, generator=gen)
    rays = ds.__getbatch__(idx)
    u = torch.rand(B, N, device=dev, generator=gen)
    roh = ds.config["ray_origin_height"]
    preps = {
        "horizontal_mode1": ds.get_point_preprocessor("horizontal").params(
            ngp_remap=True, alt_compress=8.0),
        "raw_mode0": _lib.height_params(ds.scale, ds.offset, roh, True, 8.0, append_height=False),
        "height_mode2": _lib.height_params(ds.scale, ds.offset, roh, True, 8.0),
    }
    out["fused_sampler"] = _time(
        {k: (lambda p=p: sample_and_preprocess(rays, N, p, u=u)) for k, p in preps.items()},
        a.reps)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
