"""Numbers of DESIGN.md 3.1 (profiles/tcnn_module_ref16.json, "timing"):
anr_grad_quantize_add_f16 against the three-pass composition it replaces, and the unfused /
fused reference-numerics train step at 8,192 x 1,024.

    python tools/tcnn_module_timing.py OUT.json [entry] [steps]
"""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "atmospheric-neural-rendering_amd")]

import __graft_entry__ as ge  # noqa: E402
from atmonr_amd import _lib  # noqa: E402

dev = torch.device("cuda:0")
OUT = {}


def events(fn, reps, warm=5):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    ts.sort()
    return {"median_ms": ts[len(ts) // 2], "min_ms": ts[0], "max_ms": ts[-1], "reps": reps}


def entry_points():
    enc = ge._ingp_config(64)["instant_ngp"]["encoding"]
    for log2_T in (int(enc["log2_hashmap_size"]), 21):
        n = int(_lib.hashgrid_desc(3, enc["n_levels"], enc["n_features_per_level"],
                                   enc["base_resolution"], enc["per_level_scale"],
                                   log2_T).n_params)
        g = torch.Generator(device=dev).manual_seed(1)
        src = torch.randn(n, device=dev, generator=g) * 1e-3
        scratch = src.clone()
        grad = torch.randn(n, device=dev, generator=g)
        s = _lib.stream(dev)

        def new():  # scratch holds the scatter's sums; left zeroed
            _lib.call("anr_grad_quantize_add_f16", scratch.data_ptr(), grad.data_ptr(), n, 128.0, s)

        def old():  # zero fill of a fresh buffer (the scatter target), round in place, add
            buf = torch.zeros(n, device=dev)
            _lib.call("anr_grad_quantize_f16", buf.data_ptr(), n, 128.0, s)
            grad.add_(buf)

        rec = {"n_params": n, "mbytes_f32": n * 4 / 1e6}
        # alternate the two, three rounds
        rounds = []
        for _ in range(3):
            rounds.append({"new": events(new, 20), "three_pass": events(old, 20)})
        rec["rounds"] = rounds
        with _lib.KernelTimer(only={"anr_grad_quantize_add_f16", "anr_grad_quantize_f16"}) as kt:
            for _ in range(20):
                new()
                old()
        rec["kernel_timer"] = kt.summary()
        # the parts of the three-pass form on their own
        buf = torch.zeros(n, device=dev)
        rec["zero_fill"] = events(lambda: torch.zeros(n, device=dev), 20)
        rec["torch_add_"] = events(lambda: grad.add_(buf), 20)
        OUT[f"quantize_add_log2T_{log2_T}"] = rec
        print(log2_T, json.dumps(rec), flush=True)
        del src, scratch, grad, buf


def steps():
    from atmonr_amd.batch_loader import BatchLoader
    from atmonr_amd.datasets.synthetic import SyntheticHARP2Dataset
    from atmonr_amd.pipelines.instant_ngp import InstantNGPPipeline

    B, N, WARM, STEPS = 8192, 1024, 10, 20
    opt_cfg = {"lr": 1e-2, "betas": [0.9, 0.99], "eps": 1e-15, "weight_decay": 1e-2}
    ds = SyntheticHARP2Dataset(n_views=8, img_size=256, device=dev, seed=0)
    for name, fused in (("unfused_reference", False), ("fused_reference", True)):
        p = InstantNGPPipeline(ge._ingp_config(N), ds, dtype=torch.float16, fused=fused, seed=5,
                               numerics="reference")
        p.send_tensors_to(dev)
        opt = p.get_optimizer(opt_cfg)
        it = iter(BatchLoader(ds, B, seed=1))
        ts, losses = [], []
        torch.cuda.reset_peak_memory_stats(dev)
        for k in range(WARM + STEPS):
            b = next(it)
            a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            loss = p.compute_loss(b, p.forward(b))
            opt.zero_grad()
            loss.backward()
            opt.step()
            e.record()
            torch.cuda.synchronize()
            if k >= WARM:
                ts.append(a.elapsed_time(e))
            losses.append(loss.item())
        ts.sort()
        OUT["step_" + name] = {"rays": B, "samples": N, "warmup": WARM, "steps": STEPS,
                               "median_ms": ts[len(ts) // 2], "min_ms": ts[0], "max_ms": ts[-1],
                               "mean_ms": sum(ts) / len(ts), "loss_first": losses[0],
                               "loss_last": losses[-1], "zero_rays": p.zero_rays_total,
                               "peak_mem_gb": torch.cuda.max_memory_allocated(dev) / 1e9}
        print(name, json.dumps(OUT["step_" + name]), flush=True)
        del p, opt
        torch.cuda.empty_cache()


if __name__ == "__main__":
    out_path = sys.argv[1]
    which = sys.argv[2:] or ["entry", "steps"]
    if "entry" in which:
        entry_points()
    if "steps" in which:
        steps()
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(OUT, f, indent=1)
