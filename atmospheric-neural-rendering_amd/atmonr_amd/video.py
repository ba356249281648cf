"""Orbit video of an extracted volume (the reference's scripts/make_video.py).

The reference turns the extract's extinction cube into a VDB file, shells out to OpenVDB's
``vdb_render`` (a CPU single-scattering ray marcher) once per frame of an orbit, and stitches
the frames with ffmpeg. Here the cube stays a dense tensor and the frames are marched on the
GPU by ``anr_volume_render`` (csrc/volume_render.hip; the arithmetic is defined in
include/anr.h and restated in tests/volume_checks.py). The defaults are vdb_render's and the
script's; parity with vdb_render: unpinned. No VDB file is written, and nothing is fetched:
ffmpeg runs only if a binary is already on PATH, otherwise the frames stay as PPM files.

Shadows: ``shadows="marched"`` (the default) casts a shadow march at every primary sample.
``shadows="light_volume"`` is a second, opt-in mode: the light does not move during an orbit,
so the shadow optical depth of every voxel is summed once (:func:`light_volume`,
``anr_volume_light``) and interpolated at each primary sample (``anr_volume_render_lit``). An
interpolated shadow is not a marched one: the mode has its own definition in include/anr.h and
its own yardstick (tests/light_volume_checks.py); the alpha channel is the marched mode's bit
for bit, the colours differ. Parity with vdb_render: unpinned.
"""

from __future__ import annotations

import math
import os
import shutil
import subprocess
from dataclasses import dataclass
from pathlib import Path

import numpy as np
import torch

from . import _lib
from ._lib import ANRError

# vdb_render's camera: a 41.2136 mm aperture behind a 50 mm lens
DEFAULT_HFOV = 2.0 * math.atan(41.2136 / (2.0 * 50.0))


@dataclass
class VolumeRenderSettings:
    """anr_volume_params. primary_step, shadow_step (in voxels) and light_gain are
    vdb_render's defaults; absorb, scatter, light_dir (towards the light), light_color and
    cutoff are scripts/make_video.py:79-128's."""

    absorb: tuple = (0.1, 0.1, 0.1)
    scatter: tuple = (0.7, 0.7, 0.7)
    light_dir: tuple = (0.0, 1.0, 0.0)
    light_color: tuple = (1.0, 1.0, 1.0)
    primary_step: float = 1.0
    shadow_step: float = 3.0
    light_gain: float = 0.2
    cutoff: float = 0.01

    def params(self) -> _lib.VolumeParams:
        p = _lib.VolumeParams()
        for name in ("absorb", "scatter", "light_dir", "light_color"):
            vals = tuple(float(v) for v in getattr(self, name))
            if len(vals) != 3:
                raise ANRError(f"VolumeRenderSettings.{name} needs three values")
            setattr(p, name, (_lib.c_float * 3)(*vals))
        p.primary_step, p.shadow_step = float(self.primary_step), float(self.shadow_step)
        p.light_gain, p.cutoff = float(self.light_gain), float(self.cutoff)
        return p


SHADOWS = ("marched", "light_volume")


def check_shadows(shadows) -> bool:
    """True for the light-volume mode; ValueError for a name that is neither mode."""
    if shadows not in SHADOWS:
        raise ValueError(f"shadows must be one of {SHADOWS}, got {shadows!r}")
    return shadows == "light_volume"


def light_key(settings: VolumeRenderSettings) -> tuple:
    """What a light volume depends on besides the density: light_dir, shadow_step, light_gain
    and cutoff, as the f32 values the kernel receives."""
    vals = (*settings.light_dir, settings.shadow_step, settings.light_gain, settings.cutoff)
    return tuple(float(np.float32(v)) for v in vals)


class LightVolume:
    """The shadow optical depth ``tau`` of every voxel of one volume under one light: a tensor
    of the cube's shape (dense) or of the values' (sparse), with the ``key``
    (:func:`light_key`) of the settings it was built for. Valid only for the density it was
    built from; the renders refuse it under settings with another key."""

    def __init__(self, tau: torch.Tensor, key: tuple) -> None:
        self.tau, self.key = tau, tuple(key)

    def check(self, settings: VolumeRenderSettings, shape, device) -> None:
        if self.key != light_key(settings):
            raise ANRError("the light volume was built for other settings (light_dir, "
                           f"shadow_step, light_gain, cutoff) = {self.key}, the render asks "
                           f"for {light_key(settings)}")
        if tuple(self.tau.shape) != tuple(shape) or self.tau.device != device:
            raise ANRError(f"the light volume has shape {tuple(self.tau.shape)} on "
                           f"{self.tau.device}, the volume {tuple(shape)} on {device}")


def _check_density(density: torch.Tensor, who: str) -> None:
    if not density.is_cuda:
        raise ANRError(f"{who} needs GPU tensors (got a CPU tensor)")
    if density.dim() != 3 or density.dtype != torch.float32:
        raise ANRError(f"density must be (nx, ny, nz) float32, got {tuple(density.shape)} "
                       f"{density.dtype}")


def light_volume(density: torch.Tensor,
                 settings: VolumeRenderSettings | None = None) -> LightVolume:
    """``anr_volume_light`` of the (nx, ny, nz) f32 cube ``density``: the :class:`LightVolume`
    that ``render_volume(..., shadows="light_volume", light=...)`` takes. Build it once per
    video; it holds as long as the density and the settings' light_dir, shadow_step,
    light_gain and cutoff do. CPU tensors raise ANRError."""
    settings = VolumeRenderSettings() if settings is None else settings
    _check_density(density, "light_volume")
    density = density.contiguous()
    tau = torch.empty_like(density)
    nx, ny, nz = density.shape
    with torch.cuda.device(density.device):
        _lib.call("anr_volume_light", _lib.ptr(density), nx, ny, nz, settings.params(),
                  _lib.ptr(tau), _lib.stream(density.device))
    return LightVolume(tau, light_key(settings))


def volume_from_extract(extinction, band: int = 2, scene_scale: float = 1000.0) -> np.ndarray:
    """The density cube of scripts/make_video.py:146-152 from an extract's extinction.

    ``extinction``: (H, W, A, bands), or the path of the ``.npz`` that
    ``GridExtractDataset.dump`` writes (key ``extinction``). Band ``band`` is taken, the
    altitude axis flipped, the axes transposed to (W, A, H) so that altitude is y, the values
    multiplied by ``scene_scale / 1000`` (pass the dataset's ``scale``; the default leaves
    them as they are) and NaN set to 0, VDB's background. Returns a contiguous f32 array.

    The reference parses ``--render-band-idx`` and then hard-codes band 2; here ``band`` is
    honoured and defaults to 2.
    """
    if isinstance(extinction, (str, os.PathLike)):
        with np.load(extinction, allow_pickle=False) as f:
            extinction = f["extinction"]
    if isinstance(extinction, torch.Tensor):
        extinction = extinction.detach().cpu().numpy()
    ext = np.asarray(extinction)
    if ext.ndim != 4:
        raise ANRError(f"extinction must be (H, W, A, bands), got shape {ext.shape}")
    if not -ext.shape[3] <= band < ext.shape[3]:
        raise ANRError(f"band {band} of an extinction with {ext.shape[3]} bands")
    sigma = ext[:, :, ::-1, band]
    sigma = np.transpose(sigma, (1, 2, 0)).astype(np.float64) * (scene_scale / 1000.0)
    return np.ascontiguousarray(np.nan_to_num(sigma, nan=0.0).astype(np.float32))


def look_at_camera(eye, target, up, width: int, height: int,
                   hfov: float = DEFAULT_HFOV) -> np.ndarray:
    """One anr_camera as 12 f64 numbers: eye, forward, right scaled by tan(hfov / 2), up
    scaled by tan(hfov / 2) * height / width."""
    eye, target, up = (np.asarray(v, dtype=np.float64) for v in (eye, target, up))
    fwd = target - eye
    fwd = fwd / np.linalg.norm(fwd)
    right = np.cross(fwd, up)
    if not np.linalg.norm(right) > 0.0:
        raise ANRError("look_at_camera: up is parallel to the viewing direction")
    right = right / np.linalg.norm(right)
    upv = np.cross(right, fwd)
    th = math.tan(hfov / 2.0)
    return np.concatenate([eye, fwd, right * th, upv * (th * height / width)])


def orbit_cameras(shape, duration: float = 10.0, frame_rate: int = 60, width: int = 640,
                  height: int = 480, hfov: float = DEFAULT_HFOV,
                  device: torch.device | str = "cuda") -> torch.Tensor:
    """The orbit of scripts/make_video.py:155-169 around a cube of ``shape`` = (nx, ny, nz):
    ``n = int(duration * frame_rate)`` frames at ``linspace(0, duration, n)``, radius
    ``1.3 * |shape|``, eye ``(cos * R + cx, 0.5 * |shape|, sin * R + cz)`` looking at
    ``(cx, 0, cz)`` with up (0, 1, 0), (cx, cz) = (nx / 2, nz / 2). The first and the last
    frame coincide, as the script's do. Returns (n, 12) f32 on ``device``; the maths is f64
    on the host. ``width`` and ``height`` enter through the aspect ratio alone."""
    n = int(duration * frame_rate)
    if n < 1 or duration <= 0:
        raise ANRError(f"orbit_cameras: no frames (duration {duration}, frame rate {frame_rate})")
    shape = tuple(float(s) for s in shape)
    times = np.linspace(0.0, duration, n)
    norm = float(np.linalg.norm(shape))
    cx, cz = shape[0] / 2.0, shape[2] / 2.0
    ang = 2.0 * np.pi * times / duration
    cams = np.stack([
        look_at_camera((math.cos(a) * 1.3 * norm + cx, 0.5 * norm, math.sin(a) * 1.3 * norm + cz),
                       (cx, 0.0, cz), (0.0, 1.0, 0.0), width, height, hfov)
        for a in ang])
    return torch.from_numpy(cams.astype(np.float32)).to(device)


def render_volume(density: torch.Tensor, cameras: torch.Tensor, width: int = 640,
                  height: int = 480, settings: VolumeRenderSettings | None = None,
                  max_bytes: int = 1 << 28, shadows: str = "marched",
                  light: LightVolume | None = None) -> torch.Tensor:
    """(F, height, width, 4) f32 RGBA on the device: ``anr_volume_render`` of the (nx, ny, nz)
    f32 cube ``density`` from the (F, 12) f32 ``cameras``. The frames go to the kernel in
    chunks whose output stays under ``max_bytes`` (at least one frame per launch); frames are
    independent, so the chunking does not change a bit. CPU tensors raise ANRError.

    ``shadows="light_volume"``: ``anr_volume_render_lit`` with ``light``, a
    :func:`light_volume` of this density under these settings (built here, for this call
    alone, when None; one built for other settings raises ANRError). An unknown ``shadows``
    raises ValueError."""
    lit = check_shadows(shadows)
    settings = VolumeRenderSettings() if settings is None else settings
    if not (density.is_cuda and cameras.is_cuda):
        raise ANRError("render_volume needs GPU tensors (got a CPU tensor)")
    if density.dim() != 3 or density.dtype != torch.float32:
        raise ANRError(f"density must be (nx, ny, nz) float32, got {tuple(density.shape)} "
                       f"{density.dtype}")
    if cameras.dim() != 2 or cameras.shape[1] != 12 or cameras.dtype != torch.float32:
        raise ANRError(f"cameras must be (F, 12) float32, got {tuple(cameras.shape)} "
                       f"{cameras.dtype}")
    if cameras.device != density.device:
        raise ANRError("density and cameras must be on one device")
    density, cameras = density.contiguous(), cameras.contiguous()
    F = cameras.shape[0]
    out = torch.empty((F, height, width, 4), dtype=torch.float32, device=density.device)
    if out.numel() == 0:
        return out
    params = settings.params()
    chunk = max(1, int(max_bytes) // (height * width * 16))
    nx, ny, nz = density.shape
    if lit:
        light = light_volume(density, settings) if light is None else light
        light.check(settings, density.shape, density.device)
        tau = light.tau.contiguous()
    with torch.cuda.device(density.device):
        for f0 in range(0, F, chunk):
            n = min(chunk, F - f0)
            if lit:
                _lib.call("anr_volume_render_lit", _lib.ptr(density), _lib.ptr(tau), nx, ny, nz,
                          _lib.ptr(cameras[f0:f0 + n]), n, height, width, params,
                          _lib.ptr(out[f0:f0 + n]), _lib.stream(density.device))
            else:
                _lib.call("anr_volume_render", _lib.ptr(density), nx, ny, nz,
                          _lib.ptr(cameras[f0:f0 + n]), n, height, width, params,
                          _lib.ptr(out[f0:f0 + n]), _lib.stream(density.device))
    return out


def write_ppm(path, rgb) -> None:
    """Binary P6 of an (H, W, >= 3) image: the first three channels clamped to [0, 1] and
    rounded to 8 bits."""
    if isinstance(rgb, torch.Tensor):
        rgb = rgb.detach().cpu().numpy()
    rgb = np.asarray(rgb, dtype=np.float64)
    if rgb.ndim != 3 or rgb.shape[2] < 3:
        raise ANRError(f"write_ppm: image must be (H, W, >= 3), got {rgb.shape}")
    img = np.nan_to_num(rgb[:, :, :3], nan=0.0)
    img = np.rint(np.clip(img, 0.0, 1.0) * 255.0).astype(np.uint8)
    with open(path, "wb") as f:
        f.write(b"P6\n%d %d\n255\n" % (img.shape[1], img.shape[0]))
        f.write(np.ascontiguousarray(img).tobytes())


def read_ppm(path) -> np.ndarray:
    """(H, W, 3) uint8 of a binary P6 file as write_ppm writes it."""
    with open(path, "rb") as f:
        data = f.read()
    parts = data.split(b"\n", 3)
    if len(parts) != 4 or parts[0] != b"P6" or parts[2] != b"255":
        raise ANRError(f"{path}: not a binary P6 file with 8-bit samples")
    w, h = (int(v) for v in parts[1].split())
    return np.frombuffer(parts[3], dtype=np.uint8, count=w * h * 3).reshape(h, w, 3)


def stitch_frames(result: dict, out_dir, video_path, frame_rate: int, width: int,
                  height: int) -> dict:
    """The script's ffmpeg call over ``out_dir``'s ``%06d.ppm`` frames, if a ``video_path`` is
    given and an ``ffmpeg`` binary is already on PATH; fills ``result["video"]`` and
    ``result["ffmpeg"]`` (what happened) and returns ``result``."""
    out_dir = Path(out_dir)
    ffmpeg = shutil.which("ffmpeg")
    if video_path is None:
        result["ffmpeg"] = "not asked for (no video_path); the frames stay"
    elif ffmpeg is None:
        result["ffmpeg"] = "no ffmpeg binary on PATH; the frames stay"
    else:
        cmd = [ffmpeg, "-framerate", str(frame_rate), "-i", str(out_dir / "%06d.ppm"), "-c:v",
               "libx264", "-pix_fmt", "yuv420p", "-s", f"{width}x{height}", "-y",
               str(video_path)]
        rc = subprocess.run(cmd, stdout=subprocess.DEVNULL, stderr=subprocess.STDOUT).returncode
        if rc == 0:
            result["video"] = str(video_path)
            result["ffmpeg"] = "ok"
        else:
            result["ffmpeg"] = f"ffmpeg exited with status {rc}; the frames stay"
    return result


def make_video(extract, out_dir, video_path=None, band: int = 2, scene_scale: float = 1000.0,
               width: int = 640, height: int = 480, duration: float = 10.0,
               frame_rate: int = 60, settings: VolumeRenderSettings | None = None,
               device: torch.device | str = "cuda", max_bytes: int = 1 << 28,
               shadows: str = "marched", light: LightVolume | None = None) -> dict:
    """scripts/make_video.py:142-199: the extract's cube, an orbit around it, one frame per
    camera written to ``out_dir`` as ``%06d.ppm`` (the script's temp-frame naming), and, with
    a ``video_path`` and an ``ffmpeg`` binary already on PATH, the script's ffmpeg call.
    ``extract``: what volume_from_extract takes. Returns ``{"frames": [paths], "shape": cube
    shape, "video": path or None, "ffmpeg": what happened}``; without ffmpeg the frames stay
    and ``"ffmpeg"`` says so. ``shadows="light_volume"``: the light volume is built once for
    the whole video (or ``light`` is taken, if it was built for these settings)."""
    lit = check_shadows(shadows)
    cube = volume_from_extract(extract, band=band, scene_scale=scene_scale)
    density = torch.from_numpy(cube).to(device)
    if lit and light is None:
        light = light_volume(density, settings)
    cameras = orbit_cameras(cube.shape, duration, frame_rate, width, height, device=device)
    out_dir = Path(out_dir)
    out_dir.mkdir(parents=True, exist_ok=True)
    frames = []
    per_frame = max(1, height * width * 16)
    chunk = max(1, int(max_bytes) // per_frame)
    for f0 in range(0, cameras.shape[0], chunk):
        rgba = render_volume(density, cameras[f0:f0 + chunk], width, height, settings, max_bytes,
                             shadows=shadows, light=light if lit else None)
        for k, img in enumerate(rgba.cpu().numpy()):
            frames.append(str(out_dir / f"{f0 + k:06d}.ppm"))
            write_ppm(frames[-1], img)
    result = {"frames": frames, "shape": tuple(cube.shape), "video": None}
    return stitch_frames(result, out_dir, video_path, frame_rate, width, height)
