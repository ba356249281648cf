"""Build time, size and time per frame of the sparse volume of a global-grid extract
(csrc/sparse_volume.hip), with its brick level on and off, and against the dense marcher on a
grid both can take.

    python tools/sparse_volume_timing.py [--out profiles/sparse_volume.json]

Scene: the default synthetic scene's global grid as tools/globalgrid_timing.py builds it (90
views x 512 x 512 pixels, vstretch 12, scale 100 / EARTH_RADIUS, grid_res 0.025: a 973 x 873
x 791 box with 78.3 M voxels). Values: the scene's own cloud field (extinction_truth, five
Gaussian blobs) at the voxel centres, in 1/m, times the voxel edge as
GlobalGridExtractDataset.volume applies it; no trained model is involved.

Frames: 640 x 480, the settings of global_settings (the light along the local vertical),
``--poses`` cameras of global_orbit_cameras spread over the whole circle. Every frame is one
launch between two device events. The arms (brick level on, off; at the coarser grid also the
dense marcher on the densified cube) alternate frame by frame within one process, after one
warm-up pass of every arm over every pose; the median, minimum and maximum over poses x
``--reps`` are reported per arm, and the outputs of the arms are asserted bit-equal. The
share of samples the brick level answers comes from the kernel's own counters in a separate,
untimed pass.

Comparison with the dense marcher: the same scene at grid_res 0.05, whose densified cube stays
under anr_volume_render's 2^31-byte limit. There is no vdb_render to compare with: no speed-up
over it is claimed, and parity with it stays unpinned.

Shadows: ``--shadows light_volume`` times the light-volume mode instead (SparseVolume.light
once, anr_sparse_volume_render_lit per frame) against the marched mode in the same process at
``--grid-res``, brick level on, the two arms alternating pose by pose (tools/
volume_render_timing.py's shadow_modes): per-frame time of both, the light build's time, the
break-even frame count and the RGB difference between the modes. The record goes under
"global_grid" into ``--light-out`` (profiles/light_volume.json), beside what is already there.

Registers and scratch are read from hipcc's -Rpass-analysis=kernel-resource-usage remarks for
csrc/sparse_volume.hip when hipcc is installed.
"""

from __future__ import annotations

import argparse
import json
import os
import re
import shutil
import statistics
import subprocess
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "atmospheric-neural-rendering_amd"))

W, H = 640, 480


def _stats(xs):
    return {"median_ms": statistics.median(xs), "min_ms": min(xs), "max_ms": max(xs), "n": len(xs)}


def _timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def cloud_sigma(scene, xyz: torch.Tensor, chunk: int = 1 << 22) -> torch.Tensor:
    """The scene's cloud field at WGS-84 Cartesian points (n, 3) f64: (n,) f32 in 1/m."""
    from atmonr_amd.geospatial.wgs_84 import cartesian_to_horizontal

    out = torch.empty(xyz.shape[0], dtype=torch.float32, device=xyz.device)
    for s in range(0, xyz.shape[0], chunk):
        p = xyz[s:s + chunk]
        lat, lon, alt = cartesian_to_horizontal(p[:, 0], p[:, 1], p[:, 2])
        out[s:s + chunk] = (scene.extinction_truth(lat, lon, alt) / 1000.0).float()
    return out


def grid_volume(scene, grid_res: float, vstretch: float, build_reps: int):
    """(dataset, sigma, volume, build times) of the scene's global grid at ``grid_res``."""
    from atmonr_amd.extract import GlobalGridExtractDataset
    from atmonr_amd.geospatial.spherical import EARTH_RADIUS
    from atmonr_amd.sparse_volume import SparseVolume

    ds = GlobalGridExtractDataset(scene, 100 / EARTH_RADIUS, grid_res, vstretch)
    sigma = cloud_sigma(scene, ds.xyz)
    edge = ds.grid_res / ds.scale
    build = []
    for rep in range(build_reps + 1):  # pass 0 warms up (code objects, the allocator)
        vol = None
        ms, vol = _timed(lambda: SparseVolume.from_voxels(ds.voxels, sigma, edge))
        if rep:
            build.append(ms)
    return ds, sigma, vol, build


def frames(arms: dict, cams: torch.Tensor, reps: int):
    """Per-arm list of ms per frame, the arms alternating frame by frame; the arms' outputs
    are asserted bit-equal on every pose of the warm-up pass."""
    ms = {k: [] for k in arms}
    for rep in range(reps + 1):
        for f in range(cams.shape[0]):
            first = None
            for name, fn in arms.items():
                t, img = _timed(lambda: fn(cams[f:f + 1]))
                if rep:
                    ms[name].append(t)
                elif first is None:
                    first = img
                else:
                    assert torch.equal(img, first), (name, f)
    return ms


def kernel_resources() -> dict:
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    src = os.path.join(ROOT, "atmospheric-neural-rendering_amd", "csrc", "sparse_volume.hip")
    if not os.path.exists(hipcc):
        return {"note": "hipcc not installed: not recorded"}
    cmd = [hipcc, "-O3", "-std=c++17", "--offload-arch=gfx950", "--cuda-device-only",
           "-Rpass-analysis=kernel-resource-usage", "-c", src, "-o", os.devnull]
    text = subprocess.run(cmd, capture_output=True, text=True).stderr
    out, name = {}, None
    for line in text.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            if shutil.which("c++filt"):
                filt = subprocess.run(["c++filt", name], capture_output=True, text=True)
                name = (filt.stdout.strip() or name).split("(")[0]
            out[name] = {}
        for key, pat in (("vgprs", r" VGPRs: (\d+)"), ("sgprs", r"TotalSGPRs: (\d+)"),
                         ("scratch_bytes_per_lane", r"ScratchSize \[bytes/lane\]: (\d+)"),
                         ("waves_per_simd", r"Occupancy \[waves/SIMD\]: (\d+)")):
            m = re.search(pat, line)
            if m and name:
                out[name][key] = int(m.group(1))
    return out


def measure(scene, grid_res, args, with_dense: bool) -> dict:
    from atmonr_amd.sparse_volume import (global_orbit_cameras, global_settings,
                                          render_sparse_volume)
    from atmonr_amd.video import render_volume

    t0 = time.perf_counter()
    ds, sigma, vol, build = grid_volume(scene, grid_res, args.vstretch, args.build_reps)
    torch.cuda.synchronize()
    n_box = vol.ext[0] * vol.ext[1] * vol.ext[2]
    print(f"grid_res {grid_res}: box {vol.ext}, {len(vol)} voxels, build {build} ms, "
          f"{time.perf_counter() - t0:.1f} s in all", flush=True)
    settings = global_settings(vol)
    # one more pose than asked for: the orbit's last pose repeats its first
    cams = global_orbit_cameras(vol, float(args.poses + 1), 1, W, H)[:args.poses]
    arms = {"bricks_on": lambda c: render_sparse_volume(vol, c, W, H, settings, skip=True),
            "bricks_off": lambda c: render_sparse_volume(vol, c, W, H, settings, skip=False)}
    out = {"grid_res": grid_res, "voxel_edge_m": vol.density_scale, "box": {"lo": list(vol.lo),
           "extent": list(vol.ext)}, "voxels": len(vol), "occupied": len(vol) / n_box,
           "dense_cube_bytes_derived": n_box * 4, "bytes_measured": vol.nbytes,
           "nonzero_values": float((vol.values > 0).float().mean()),
           "build_ms": _stats(build), "poses": args.poses, "image": [W, H]}
    if with_dense:
        rel = (ds.voxels - torch.tensor(vol.lo, device=ds.voxels.device, dtype=torch.int32)).long()
        cube = torch.zeros(vol.ext, dtype=torch.float32, device=vol.device)
        cube[rel[:, 0], rel[:, 1], rel[:, 2]] = (sigma.double() * vol.density_scale).float()
        out["dense_cube_bytes_measured"] = cube.numel() * cube.element_size()
        arms["dense"] = lambda c: render_volume(cube, c, W, H, settings)
    ms = frames(arms, cams, args.reps)
    out["ms_per_frame"] = {k: _stats(v) for k, v in ms.items()}
    out["ms_per_frame_by_pose"] = {
        k: [statistics.median(v[p::args.poses]) for p in range(args.poses)] for k, v in ms.items()}
    out["outputs_bit_equal"] = True  # asserted in frames()
    counters = torch.zeros(2, dtype=torch.int64, device=vol.device)
    img = render_sparse_volume(vol, cams, W, H, settings, skip=True, counters=counters)
    samples, skipped = counters.tolist()
    out["samples_in_box"] = samples
    out["samples_answered_by_bricks"] = skipped
    out["share_answered_by_bricks"] = skipped / max(1, samples)
    out["mean_alpha"] = float(img[..., 3].mean())
    out["lit_pixels"] = float((img[..., :3].amax(dim=-1) > 20 / 255).float().mean())
    print(json.dumps({k: out[k] for k in ("ms_per_frame", "share_answered_by_bricks",
                                          "mean_alpha", "bytes_measured")}), flush=True)
    return out


def shadows_arm(scene, args) -> dict:
    from atmonr_amd.sparse_volume import (global_orbit_cameras, global_settings,
                                          render_sparse_volume)

    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from volume_render_timing import shadow_modes

    ds, sigma, vol, build = grid_volume(scene, args.grid_res, args.vstretch, 1)
    settings = global_settings(vol)
    warmup = 2
    cams = global_orbit_cameras(vol, float(args.poses + warmup + 1), 1, W, H)[:args.poses + warmup]

    def build_light():
        vol._light = None  # a fresh build, not the kept one
        return vol.light(settings)

    out = shadow_modes(lambda c: render_sparse_volume(vol, c, W, H, settings),
                       lambda c, light: render_sparse_volume(vol, c, W, H, settings,
                                                             shadows="light_volume", light=light),
                       build_light, cams, warmup)
    out.update({"grid_res": args.grid_res, "box": list(vol.ext), "voxels": len(vol),
                "image": [W, H], "poses": args.poses, "volume_bytes": vol.nbytes,
                "enumeration": "one thread per value; the voxel found by a binary search of "
                               "the ranks (the only enumeration built and measured)",
                "settings": "global_settings: the light along the local vertical"})
    return out


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=90)
    ap.add_argument("--img", type=int, default=512)
    ap.add_argument("--vstretch", type=float, default=12.0)
    ap.add_argument("--grid-res", type=float, default=0.025)
    ap.add_argument("--compare-grid-res", type=float, default=0.05)
    ap.add_argument("--poses", type=int, default=8)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--build-reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sparse_volume.json"))
    ap.add_argument("--shadows", choices=("marched", "light_volume"), default="marched")
    ap.add_argument("--light-out", default=os.path.join(ROOT, "profiles", "light_volume.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("sparse_volume_timing needs a GPU: nothing here can be timed without one")
    from atmonr_amd.datasets.synthetic import SyntheticHARP2Dataset

    dev = torch.device("cuda:0")
    scene = SyntheticHARP2Dataset(n_views=args.views, img_size=args.img, device=dev)
    if args.shadows == "light_volume":
        sys.path.insert(0, os.path.join(ROOT, "tools"))
        from volume_render_timing import merge_record

        rec = shadows_arm(scene, args)
        print(json.dumps(merge_record(args.light_out, "global_grid", rec), indent=1))
        return
    out = {"gpu": torch.cuda.get_device_name(0), "parity_with_vdb_render": "unpinned",
           "scene": {"views": args.views, "img": args.img, "vstretch": args.vstretch,
                     "values": "the scene's extinction_truth at the voxel centres, 1/m, times the "
                               "voxel edge"},
           "global_grid": measure(scene, args.grid_res, args, with_dense=False),
           "against_dense": measure(scene, args.compare_grid_res, args, with_dense=True),
           "kernel_resources": kernel_resources(),
           "measured_and_derived": "every *_ms, bytes_measured, dense_cube_bytes_measured, the "
                                   "sample counts and the shares are measured; "
                                   "dense_cube_bytes_derived is extent product x 4",
           "comparison": "no vdb_render on these machines: no speed-up over it is claimed"}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
