"""Accuracy and time per frame of the volume ray marcher (anr_volume_render) on the GPU.

    python tools/volume_render_timing.py [--out profiles/volume_render.json]

Accuracy: the cases of tests/test_volume_gpu.py against the f64 numpy yardstick
(tests/volume_checks.py): per case and channel the kernel's largest error e_gpu, the error
e_arm of the yardstick's own float32 arm, and the bound max(4 e_arm, 2^-20 max|yardstick|).

Time: a synthetic cloud cube of 512 x 81 x 512 voxels (the (W, A, H) cube of a 512 x 512 x 81
extract), 640 x 480 pixels, the default settings, the cameras of the script's orbit spread over
the whole circle. Every frame is one launch between two device events; 3 warm-up frames, then
the median, minimum and maximum of 20. The library holds one layout, the cube read in place.
A second one, a zero-bordered copy of aligned z pairs, was measured against it once and
removed; its figures are kept in profiles/volume_render_layout_ab.json and copied into this
tool's output beside the fresh one. There is no parent-commit time and no vdb_render to
compare with: no speed-up over either is claimed.

Shadows: ``--shadows light_volume`` times the light-volume mode instead (anr_volume_light once,
anr_volume_render_lit per frame) against the marched mode in the same process, the two arms
alternating frame by frame on the cube and cameras above: per-frame time of both, the light
build's time, the break-even frame count (build / saving per frame), and the largest and mean
RGB difference between the modes (alpha is asserted bit-equal). The record goes under
"dense_cube" into ``--light-out`` (profiles/light_volume.json), beside what is already there.

Lookups: D evaluations per frame, counted by the yardstick's model on a downscaled case (the
same cloud at 64 x 10 x 64, 20 x 15 pixels, steps scaled by 1 / 8), as lookups per pixel.
"""

from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "atmospheric-neural-rendering_amd"))


def cloud_cube(nx: int, ny: int, nz: int, seed: int = 0, device="cpu") -> torch.Tensor:
    """A few dozen Gaussian puffs in a layer, densities up to about 0.3, zero elsewhere."""
    g = torch.Generator().manual_seed(seed)
    n = 40
    c = torch.rand(n, 3, generator=g) * torch.tensor([1.0, 0.5, 1.0]) + torch.tensor([0.0, 0.2, 0.0])
    r = 0.02 + 0.05 * torch.rand(n, generator=g)
    a = 0.1 + 0.2 * torch.rand(n, generator=g)
    c, r, a = c.to(device), r.to(device), a.to(device)
    x = (torch.arange(nx, device=device) + 0.5) / nx
    y = (torch.arange(ny, device=device) + 0.5) / ny
    z = (torch.arange(nz, device=device) + 0.5) / nz
    den = torch.zeros(nx, ny, nz, device=device)
    for k in range(n):
        ex = torch.exp(-0.5 * ((x - c[k, 0]) / r[k]) ** 2)
        ey = torch.exp(-0.5 * ((y - c[k, 1]) / (2.0 * r[k])) ** 2)
        ez = torch.exp(-0.5 * ((z - c[k, 2]) / r[k]) ** 2)
        den = torch.maximum(den, a[k] * ex[:, None, None] * ey[None, :, None] * ez[None, None, :])
    den[den < 0.005] = 0.0
    return den.float().contiguous()


def accuracy(dev) -> dict:
    from atmonr_amd.video import VolumeRenderSettings, render_volume
    from tests import volume_checks as vc

    out = {}
    for name in vc.CASES:
        den, cams, H, W, P = vc.case(name)
        s = VolumeRenderSettings(**{k: getattr(P, k) for k in P.__dataclass_fields__})
        got = render_volume(torch.from_numpy(den).to(dev), torch.from_numpy(cams).to(dev), W, H, s)
        e_gpu, e_arm, bound = vc.errors(name, got.cpu().numpy())
        keep = vc.compared_pixels(name)
        out[name] = {"e_gpu": e_gpu.tolist(), "e_arm": e_arm.tolist(), "bound": bound.tolist(),
                     "compared_pixels": int(keep.sum()), "pixels": int(keep.size),
                     "within_bound": bool(np.all(e_gpu <= bound))}
        print(name, out[name], flush=True)
    return out


def lookups_model() -> dict:
    from tests import volume_checks as vc

    shape = (64, 10, 64)
    den = cloud_cube(*shape).numpy()
    H, W = 15, 20
    cams = np.stack([vc.orbit_pose(shape, f, H, W) for f in (0.0, 0.3)])
    # a voxel here is 8 voxels of the full cube: steps of 1 / 8 and 3 / 8 voxel keep the steps
    # per ray, and 8 times the coefficients and the gain keep the optical depths
    d = vc.Params()
    P8 = vc.Params(absorb=tuple(8 * a for a in d.absorb), scatter=tuple(8 * s for s in d.scatter),
                   primary_step=d.primary_step / 8, shadow_step=d.shadow_step / 8,
                   light_gain=d.light_gain * 8)
    res = vc.render(den, cams, H, W, P8)
    per_pixel = float(res["lookups"].mean())
    return {"cube": list(shape), "image": [W, H], "frames": len(cams),
            "primary_step": P8.primary_step, "shadow_step": P8.shadow_step,
            "lookups_per_pixel": per_pixel,
            "lookups_per_640x480_frame": per_pixel * 640 * 480,
            "miss_share": float(res["flags"][..., 3].mean())}


def timing(dev, frames: int, warmup: int) -> dict:
    from atmonr_amd.video import orbit_cameras, render_volume

    nx, ny, nz, W, H = 512, 81, 512, 640, 480
    den = cloud_cube(nx, ny, nz, device=dev)
    n = frames + warmup
    cams = orbit_cameras((nx, ny, nz), duration=float(n), frame_rate=1, width=W, height=H,
                         device=dev)
    ms, alpha = [], []
    for f in range(n):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        img = render_volume(den, cams[f:f + 1], W, H)
        b.record()
        b.synchronize()
        if f >= warmup:
            ms.append(a.elapsed_time(b))
            alpha.append(float(img[..., 3].mean()))
    return {"cube": [nx, ny, nz], "cube_bytes": nx * ny * nz * 4, "image": [W, H],
            "nonzero_voxels": float((den > 0).float().mean()),
            "layouts": {"in_place_bounds_checked_edges": {
                "ms_per_frame_median": statistics.median(ms), "ms_per_frame_min": min(ms),
                "ms_per_frame_max": max(ms), "frames": len(ms), "warmup_frames": warmup}},
            "layouts_not_built": ["zero border alone (no pairs)", "non-overlapping aligned pairs"],
            "mean_alpha": statistics.mean(alpha),
            "comparison": "no parent-commit time and no vdb_render on these machines: "
                          "no speed-up is claimed"}


def _event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def _stats(xs) -> dict:
    return {"median_ms": statistics.median(xs), "min_ms": min(xs), "max_ms": max(xs), "n": len(xs)}


def shadow_modes(marched, lit, build, cams, warmup: int, build_reps: int = 3) -> dict:
    """The two shadow modes frame by frame: ``marched(c)`` and ``lit(c, light)`` render the
    cameras ``c``, ``build()`` returns a fresh light volume. Shared with
    tools/sparse_volume_timing.py."""
    build_ms = []
    for rep in range(build_reps + 1):  # pass 0 warms up
        ms, light = _event_ms(build)
        if rep:
            build_ms.append(ms)
    t = {"marched": [], "light_volume": []}
    diff_max, diff_mean = [], []
    for f in range(cams.shape[0]):
        tm, a = _event_ms(lambda: marched(cams[f:f + 1]))
        tl, b = _event_ms(lambda: lit(cams[f:f + 1], light))
        assert torch.equal(a[..., 3], b[..., 3]), f  # the alpha channel is the marched one's
        if f >= warmup:
            t["marched"].append(tm)
            t["light_volume"].append(tl)
            d = (a[..., :3] - b[..., :3]).abs()
            diff_max.append(float(d.max()))
            diff_mean.append(float(d.mean()))
    out = {"ms_per_frame": {k: _stats(v) for k, v in t.items()}, "light_build_ms": _stats(build_ms),
           "light_bytes": light.tau.numel() * light.tau.element_size(),
           "rgb_difference_between_modes": {"largest": max(diff_max),
                                            "mean": statistics.mean(diff_mean)},
           "alpha_bit_equal": True, "warmup_frames": warmup}
    saved = out["ms_per_frame"]["marched"]["median_ms"] - out["ms_per_frame"]["light_volume"]["median_ms"]
    out["ms_saved_per_frame"] = saved
    out["break_even_frames"] = (int(np.ceil(out["light_build_ms"]["median_ms"] / saved))
                                if saved > 0 else None)
    out["frames_600_ms"] = {"marched": 600 * out["ms_per_frame"]["marched"]["median_ms"],
                            "light_volume": out["light_build_ms"]["median_ms"]
                            + 600 * out["ms_per_frame"]["light_volume"]["median_ms"]}
    return out


def merge_record(path: str, key: str, rec: dict) -> dict:
    out = {}
    if os.path.exists(path):
        with open(path) as f:
            out = json.load(f)
    out.update({"gpu": torch.cuda.get_device_name(0), "parity_with_vdb_render": "unpinned",
                key: rec})
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    return out


def shadows_timing(dev, frames: int, warmup: int) -> dict:
    from atmonr_amd.video import light_volume, orbit_cameras, render_volume

    nx, ny, nz, W, H = 512, 81, 512, 640, 480
    den = cloud_cube(nx, ny, nz, device=dev)
    n = frames + warmup
    cams = orbit_cameras((nx, ny, nz), duration=float(n), frame_rate=1, width=W, height=H,
                         device=dev)
    out = shadow_modes(lambda c: render_volume(den, c, W, H),
                       lambda c, light: render_volume(den, c, W, H, shadows="light_volume",
                                                      light=light),
                       lambda: light_volume(den), cams, warmup)
    out.update({"cube": [nx, ny, nz], "image": [W, H], "settings": "defaults",
                "nonzero_voxels": float((den > 0).float().mean())})
    return out


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "volume_render.json"))
    ap.add_argument("--shadows", choices=("marched", "light_volume"), default="marched")
    ap.add_argument("--light-out", default=os.path.join(ROOT, "profiles", "light_volume.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("volume_render_timing needs a GPU: nothing here can be timed without one")
    dev = torch.device("cuda:0")
    if args.shadows == "light_volume":
        rec = shadows_timing(dev, args.frames, args.warmup)
        print(json.dumps(merge_record(args.light_out, "dense_cube", rec), indent=1))
        return
    out = {"gpu": torch.cuda.get_device_name(0), "parity_with_vdb_render": "unpinned",
           "accuracy": accuracy(dev), "timing": timing(dev, args.frames, args.warmup),
           "lookups_model": lookups_model()}
    ab = os.path.join(ROOT, "profiles", "volume_render_layout_ab.json")
    if os.path.exists(ab):  # the removed pair-layout arm, as it was measured
        with open(ab) as f:
            rec = json.load(f)
        out["timing"]["layouts"]["zero_bordered_z_pairs_float2_removed"] = {
            "ms_per_frame_median": rec["pairs"]["ms_per_frame_median"],
            "ms_per_frame_min": rec["pairs"]["min"], "ms_per_frame_max": rec["pairs"]["max"],
            "frames": rec["pairs"]["frames"], "same_run_in_place_median": rec["in_place"]["ms_per_frame_median"],
            "source": "profiles/volume_render_layout_ab.json"}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
