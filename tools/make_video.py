"""Orbit video of an extracted volume, after the reference's scripts/make_video.py.

    python tools/make_video.py --extract-filepath extract.npz --video-filepath orbit.mp4

The options keep the reference script's names. The frames are marched on the GPU
(atmonr_amd.video, anr_volume_render) and written as <frames-dir>/%06d.ppm; ffmpeg stitches
them only if a binary is already on PATH, otherwise the frames stay and the tool says so.
No VDB file is written (--vdb-filepath is accepted and ignored). Parity with vdb_render:
unpinned.
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
    ap.add_argument("--extract-filepath", required=True, help="the .npz an extract dumped (key 'extinction')")
    ap.add_argument("--vdb-filepath", default=None, help="accepted for compatibility; no VDB file is written")
    ap.add_argument("--video-filepath", required=True, help="where ffmpeg writes the video, if ffmpeg is on PATH")
    ap.add_argument("--render-band-idx", type=int, default=2, help="band to render (the reference hard-codes 2)")
    ap.add_argument("--res", default="640x480", help="resolution, WIDTHxHEIGHT")
    ap.add_argument("--frame-rate", type=int, default=60, help="frames per second")
    ap.add_argument("--duration", type=float, default=10.0, help="seconds of video (one orbit)")
    ap.add_argument("--absorb", nargs=3, type=float, default=(0.1, 0.1, 0.1), help="absorption coefficients, RGB")
    ap.add_argument("--cutoff", type=float, default=0.01, help="density and transmittance cutoff")
    ap.add_argument("--light-source-dir", nargs=3, type=float, default=(0.0, 1.0, 0.0), help="direction towards the light")
    ap.add_argument("--light-source-color", nargs=3, type=float, default=(1.0, 1.0, 1.0), help="light colour, RGB")
    ap.add_argument("--scatter", nargs=3, type=float, default=(0.7, 0.7, 0.7), help="scattering coefficients, RGB")
    ap.add_argument("--scene-scale", type=float, default=1000.0, help="the dataset's scale; densities are multiplied by scale / 1000")
    ap.add_argument("--frames-dir", default="_temp_frames", help="directory of the %%06d.ppm frames")
    ap.add_argument("--shadows", choices=("marched", "light_volume"), default="marched", help="marched: a shadow march per sample; light_volume: shadows precomputed once per video and interpolated (another arithmetic, same alpha)")
    return ap


def main() -> None:
    args = build_parser().parse_args()
    if not os.path.exists(args.extract_filepath):
        sys.exit(f"{args.extract_filepath}: no such file")
    res = [int(p) for p in args.res.split("x")]
    if len(res) != 2 or res[0] <= 0 or res[1] <= 0 or args.duration <= 0:
        sys.exit("--res must be WIDTHxHEIGHT with positive sides, --duration positive")
    if res[0] * res[1] > 1920 * 1080:
        warnings.warn(f"a resolution of {res} makes every frame slow to march")
    import numpy as np

    from atmonr_amd.video import VolumeRenderSettings, make_video

    light = np.asarray(args.light_source_dir, dtype=np.float64)
    if not np.linalg.norm(light) > 0:
        sys.exit("--light-source-dir must not be the zero vector")
    settings = VolumeRenderSettings(absorb=tuple(args.absorb), scatter=tuple(args.scatter),
                                    light_dir=tuple(light / np.linalg.norm(light)),
                                    light_color=tuple(args.light_source_color),
                                    cutoff=args.cutoff)
    out = make_video(args.extract_filepath, args.frames_dir, args.video_filepath,
                     band=args.render_band_idx, scene_scale=args.scene_scale, width=res[0],
                     height=res[1], duration=args.duration, frame_rate=args.frame_rate,
                     settings=settings, shadows=args.shadows)
    out["frames"] = f"{len(out['frames'])} files under {args.frames_dir}"
    print(json.dumps(out))


if __name__ == "__main__":
    main()
