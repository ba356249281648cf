#!/usr/bin/env python
"""Time InstantNGPPipeline.render at the workload shape (8,192 rays x 1,024 samples, W = 64):
the fused kernel (anr_ingp_render, fused=True) against forward's own path under no_grad
(fused=False), in both numerics. Device events around one call, median of 20 after 10
warm-up calls, three rounds alternating the two paths. Also records
torch.cuda.max_memory_allocated over one call of each path and the build-numerics composite
error figures of tests/test_render_gpu.py (tests/render_checks.composite_errors).

Writes one record to profiles/render_fused.json (or --out). The rule for fused="auto": the
kernel serves "auto" if its median is not above the fallback's by more than the rounds' own
spread (the larger max - min of the two paths' round medians).
"""

from __future__ import annotations

import argparse
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
from tests import render_checks as rc  # noqa: E402


def _median_ms(fn, warmup, iters):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return statistics.median(times)


def _peak_bytes(fn, dev):
    fn()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(dev)
    base = torch.cuda.memory_allocated(dev)
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated(dev)
    del out
    return peak, peak - base


def main() -> None:
    from atmonr_amd.batch_loader import BatchLoader
    from atmonr_amd.datasets.synthetic import SyntheticHARP2Dataset
    from atmonr_amd.pipelines.instant_ngp import InstantNGPPipeline

    ap = argparse.ArgumentParser()
    ap.add_argument("--rays", type=int, default=8192)
    ap.add_argument("--samples", type=int, default=1024)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "render_fused.json"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    B, N = args.rays, args.samples
    scene = SyntheticHARP2Dataset(n_views=8, img_size=48, device=dev, seed=0)
    record = {"shape": [B, N], "width": 64, "dir_hidden_layers": 2,
              "device": torch.cuda.get_device_name(dev),
              "timing": f"device events, median of {args.iters} after {args.warmup} warm-up, "
                        f"{args.rounds} alternating rounds",
              "run_leader_gathers": False, "numerics": {}}
    for numerics in ("reference", "build"):
        pipe = InstantNGPPipeline(ge._ingp_config(N), scene, seed=5, numerics=numerics)
        pipe.send_tensors_to(dev)
        batch = next(iter(BatchLoader(scene, B, seed=1)))
        u = torch.rand(B, N, generator=torch.Generator().manual_seed(2)).to(dev)
        factor, _ = rc.make_alive(pipe, batch, u)
        paths = {"fused": lambda: pipe.render(batch, u=u, fused=True),
                 "forward": lambda: pipe.render(batch, u=u, fused=False)}
        rounds = {k: [] for k in paths}
        for _ in range(args.rounds):
            for k, fn in paths.items():
                rounds[k].append(_median_ms(fn, args.warmup, args.iters))
        med = {k: statistics.median(v) for k, v in rounds.items()}
        spread = max(max(v) - min(v) for v in rounds.values())
        mem = {k: dict(zip(("max_memory_allocated", "rise_bytes"), _peak_bytes(fn, dev)))
               for k, fn in paths.items()}
        for k in mem:
            mem[k]["rise_bytes_per_sample"] = mem[k]["rise_bytes"] / (B * N)
        record["numerics"][numerics] = {
            "table_factor": factor, "round_medians_ms": rounds, "median_ms": med,
            "rounds_spread_ms": spread, "memory": mem,
            "auto_takes_kernel": bool(med["fused"] <= med["forward"] + spread)}
        print(numerics, json.dumps(record["numerics"][numerics]), flush=True)
        del pipe
    errors = {}
    scene = SyntheticHARP2Dataset(n_views=8, img_size=16, device=dev, seed=0)  # the tests' scene
    for mlp_dtype in (torch.float16, torch.bfloat16):
        for (b, n) in ((40, 128), (3, 1024)):
            pipe = InstantNGPPipeline(ge._ingp_config(n), scene, seed=5, mlp_dtype=mlp_dtype)
            pipe.send_tensors_to(dev)
            batch = next(iter(BatchLoader(scene, b, seed=1)))
            u = torch.rand(b, n, generator=torch.Generator().manual_seed(2)).to(dev)
            rc.make_alive(pipe, batch, u)
            errs = rc.composite_errors(pipe, batch, u)
            errors[f"{str(mlp_dtype).split('.')[-1]}_{b}x{n}"] = {
                k: {"e_render": er, "e_forward": ef} for k, (er, ef) in errs.items()}
    record["build_composite_errors"] = errors
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(record, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
