"""Orbit video of a global-grid extract: the global view of the voxels and their extinction.

    python tools/make_global_video.py --voxels-filepath voxels.npy --sigma-filepath sigma.npy \\
        --grid-res 0.025 --video-filepath orbit.mp4

The options keep tools/make_video.py's names where they apply. The two files are what
GlobalGridExtractDataset.dump writes. They become a sparse volume on the GPU
(atmonr_amd.sparse_volume, anr_sparse_volume_render); the frames are written as
<frames-dir>/%06d.ppm, and ffmpeg stitches them only if a binary is already on PATH, otherwise
the frames stay and the tool says so. The extinction is multiplied by the voxel edge in
metres, --grid-res / --grid-scale (this project's choice: optical depth per voxel edge), and
the light shines along the local vertical unless --light-source-dir is given. No VDB file is
written. Parity with vdb_render: unpinned.
"""

from __future__ import annotations

import argparse
import json
import os
import sys
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "atmospheric-neural-rendering_amd"))


def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--voxels-filepath", required=True, help="voxels.npy of a global-grid extract, (n, 3) grid indices")
    ap.add_argument("--sigma-filepath", required=True, help="sigma.npy of the same extract, (n, bands) in 1/m")
    ap.add_argument("--grid-res", type=float, default=0.025, help="the extract's grid_res")
    ap.add_argument("--grid-scale", type=float, default=None, help="the extract's grid scale (default 100 / EARTH_RADIUS)")
    ap.add_argument("--video-filepath", required=True, help="where ffmpeg writes the video, if ffmpeg is on PATH")
    ap.add_argument("--render-band-idx", type=int, default=2, help="band to render")
    ap.add_argument("--res", default="640x480", help="resolution, WIDTHxHEIGHT")
    ap.add_argument("--frame-rate", type=int, default=60, help="frames per second")
    ap.add_argument("--duration", type=float, default=10.0, help="seconds of video (one orbit)")
    ap.add_argument("--absorb", nargs=3, type=float, default=(0.1, 0.1, 0.1), help="absorption coefficients, RGB")
    ap.add_argument("--cutoff", type=float, default=0.01, help="density and transmittance cutoff")
    ap.add_argument("--light-source-dir", nargs=3, type=float, default=None, help="direction towards the light, grid axes (default: the local vertical)")
    ap.add_argument("--light-source-color", nargs=3, type=float, default=(1.0, 1.0, 1.0), help="light colour, RGB")
    ap.add_argument("--scatter", nargs=3, type=float, default=(0.7, 0.7, 0.7), help="scattering coefficients, RGB")
    ap.add_argument("--frames-dir", default="_temp_frames", help="directory of the %%06d.ppm frames")
    ap.add_argument("--shadows", choices=("marched", "light_volume"), default="marched", help="marched: a shadow march per sample; light_volume: shadows precomputed once per video and interpolated (another arithmetic, same alpha)")
    return ap


def main() -> None:
    args = build_parser().parse_args()
    for path in (args.voxels_filepath, args.sigma_filepath):
        if not os.path.exists(path):
            sys.exit(f"{path}: no such file")
    res = [int(p) for p in args.res.split("x")]
    if len(res) != 2 or res[0] <= 0 or res[1] <= 0 or args.duration <= 0:
        sys.exit("--res must be WIDTHxHEIGHT with positive sides, --duration positive")
    if res[0] * res[1] > 1920 * 1080:
        warnings.warn(f"a resolution of {res} makes every frame slow to march")
    import numpy as np

    from atmonr_amd.sparse_volume import SparseVolume, global_settings, make_global_video

    kw = dict(absorb=tuple(args.absorb), scatter=tuple(args.scatter),
              light_color=tuple(args.light_source_color), cutoff=args.cutoff)
    if args.light_source_dir is not None:
        light = np.asarray(args.light_source_dir, dtype=np.float64)
        if not np.linalg.norm(light) > 0:
            sys.exit("--light-source-dir must not be the zero vector")
        kw["light_dir"] = tuple(light / np.linalg.norm(light))
    volume = SparseVolume.from_files(args.voxels_filepath, args.sigma_filepath,
                                     band=args.render_band_idx, grid_res=args.grid_res,
                                     grid_scale=args.grid_scale)
    out = make_global_video(volume, args.frames_dir, args.video_filepath, width=res[0],
                            height=res[1], duration=args.duration, frame_rate=args.frame_rate,
                            settings=global_settings(volume, **kw), shadows=args.shadows)
    out["frames"] = f"{len(out['frames'])} files under {args.frames_dir}"
    out["voxels"] = len(volume)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
