"""Global view of a global-grid extract: a sparse volume and its orbit video.

The reference writes the global grid (``--coord-mode globalgrid``) as a sparse OpenVDB file
for an external viewer. Here the voxels and their extinction become a :class:`SparseVolume`
on the GPU -- the traversal's own bitmap with a rank per word, the values in bitmap order and
one bit per 8 x 8 x 8 brick (csrc/sparse_volume.hip, contract in include/anr.h) -- and the
orbit frames are marched over it by ``anr_sparse_volume_render``, which is
``anr_volume_render``'s march with another source for the eight values of a sample: the
output equals the dense kernel's on the densified cube bit for bit, without that cube ever
existing (at the default grid it would be 2.69 GB). No VDB file is written. Parity with
vdb_render: unpinned.

Frame: voxel ``(i, j, k)`` of the grid sits at ``(i, j, k) - lo``, ``lo`` being the smallest
index per axis, so camera coordinates stay small in f32.

Units: the extract's extinction is in 1/m. This project multiplies it, by default, by the voxel
edge in metres (``grid_res / scale``), so that the density is optical depth per voxel edge
and the march's steps, which are in voxels, integrate it as they stand. That is this
project's choice: the reference leaves 1/m in the VDB file and the scaling to the viewer.
"""

from __future__ import annotations

import ctypes
import math
import os
from pathlib import Path

import numpy as np
import torch

from . import _lib
from ._lib import ANRError
from .video import (DEFAULT_HFOV, LightVolume, VolumeRenderSettings, check_shadows, light_key,
                    look_at_camera, stitch_frames, write_ppm)


class SparseVolume:
    """``lo`` and ``ext``: the box ``[lo, lo + ext)`` in grid indices. ``cells``
    (n_words, 2) int32 ``{bits, rank}`` per bitmap word, ``values`` (n,) f32 in ascending
    bitmap order, ``coarse`` int32 brick bits; all on one GPU. Build one with
    :meth:`from_voxels` or :meth:`from_files`."""

    def __init__(self, lo, ext, row_pitch, cells, values, coarse, density_scale) -> None:
        self.lo, self.ext, self.row_pitch = tuple(lo), tuple(ext), int(row_pitch)
        self.cells, self.values, self.coarse = cells, values, coarse
        self.density_scale = float(density_scale)
        self._light = None  # the last light volume built: (key, skip) and the LightVolume

    def __len__(self) -> int:
        return int(self.values.shape[0])

    @property
    def device(self) -> torch.device:
        return self.values.device

    @property
    def nbytes(self) -> dict:
        """Bytes of the structure on the device, part by part."""
        out = {k: getattr(self, k).numel() * getattr(self, k).element_size()
               for k in ("cells", "values", "coarse")}
        out["total"] = sum(out.values())
        return out

    def desc(self, skip: bool = True) -> _lib.SparseVolumeDesc:
        d = _lib.SparseVolumeDesc()
        d.cells, d.values = _lib.ptr(self.cells), _lib.ptr(self.values)
        d.coarse = _lib.ptr(self.coarse) if skip else None
        d.ni, d.nj, d.nk = self.ext
        d.reserved, d.row_pitch, d.n_values = 0, self.row_pitch, len(self)
        return d

    @classmethod
    def from_voxels(cls, voxels: torch.Tensor, values: torch.Tensor,
                    density_scale: float = 1.0) -> "SparseVolume":
        """``voxels`` (n, 3) integer grid indices and ``values`` (n,) on the GPU, in any order;
        the result does not depend on it. The values are multiplied by ``density_scale`` in
        f64 and rounded once to f32; NaN becomes 0. Raises ANRError for CPU tensors, n = 0,
        n >= 2^31, a box of 2^31 bitmap words or more, and duplicate voxels."""
        if not (isinstance(voxels, torch.Tensor) and isinstance(values, torch.Tensor)
                and voxels.is_cuda and values.is_cuda):
            raise ANRError("SparseVolume.from_voxels needs GPU tensors (got a CPU tensor)")
        if voxels.dim() != 2 or voxels.shape[1] != 3 or voxels.dtype.is_floating_point:
            raise ANRError(f"voxels must be (n, 3) integers, got {tuple(voxels.shape)} "
                           f"{voxels.dtype}")
        n = voxels.shape[0]
        if values.shape != (n,):
            raise ANRError(f"values must be ({n},), got {tuple(values.shape)}")
        if voxels.device != values.device:
            raise ANRError("voxels and values must be on one device")
        if n == 0:
            raise ANRError("SparseVolume.from_voxels: no voxels (n = 0)")
        if n >= 1 << 31:
            raise ANRError("SparseVolume.from_voxels: 2^31 voxels or more")
        if not math.isfinite(density_scale):
            raise ANRError(f"density_scale {density_scale} is not finite")
        lo64, hi64 = voxels.amin(dim=0).tolist(), voxels.amax(dim=0).tolist()
        if min(lo64) < -(1 << 31) or max(hi64) > (1 << 31) - 1:
            raise ANRError("voxel indices outside int32")
        voxels = voxels.to(torch.int32).contiguous()
        values = values.to(torch.float32).contiguous()
        lo = [int(v) for v in lo64]
        ext = [int(h) - int(l) + 1 for l, h in zip(lo64, hi64)]
        row_pitch = (ext[0] + 31) // 32 * 32
        n_words = row_pitch // 32 * ext[1] * ext[2]
        if max(ext) >= 1 << 31 or n_words >= 1 << 31:
            raise ANRError(f"a box of {ext} voxels takes {n_words} bitmap words: 2^31 or more")
        coarse_words = _lib.load().anr_sparse_volume_coarse_words(*ext)
        if coarse_words <= 0:
            raise ANRError(f"a box of {ext} voxels has 2^31 bricks or more")
        dev = voxels.device
        box = (*lo, *ext, row_pitch)
        with torch.cuda.device(dev):
            st = _lib.stream(dev)
            cells = torch.zeros((n_words, 2), dtype=torch.int32, device=dev)
            coarse = torch.zeros(coarse_words, dtype=torch.int32, device=dev)
            _lib.call("anr_sparse_volume_mark", _lib.ptr(voxels), n, *box, _lib.ptr(cells),
                      _lib.ptr(coarse), st)
            counts = torch.empty(n_words, dtype=torch.int32, device=dev)
            _lib.call("anr_sparse_volume_popcount", _lib.ptr(cells), n_words, _lib.ptr(counts), st)
            ends = torch.cumsum(counts, 0, dtype=torch.int64)
            total = int(ends[-1].item())
            if total != n:
                raise ANRError(f"SparseVolume.from_voxels: {n} voxels set {total} bits: "
                               "duplicate voxels")
            cells[:, 1] = (ends - counts).to(torch.int32)
            del ends, counts
            out = torch.empty(n, dtype=torch.float32, device=dev)
            _lib.call("anr_sparse_volume_place", _lib.ptr(voxels), _lib.ptr(values), n,
                      float(density_scale), *box, _lib.ptr(cells), n, _lib.ptr(out), st)
        return cls(lo, ext, row_pitch, cells, out, coarse, density_scale)

    @classmethod
    def from_files(cls, voxels_npy, sigma_npy, band: int = 2, density_scale: float | None = None,
                   grid_res: float | None = None, grid_scale: float | None = None,
                   device: torch.device | str = "cuda") -> "SparseVolume":
        """The ``voxels.npy`` (n, 3) and ``sigma.npy`` (n, bands) that
        ``GlobalGridExtractDataset.dump`` writes; arrays are taken as well. Band ``band`` is
        rendered (the reference parses ``--render-band-idx`` and then hard-codes 2; here it is
        honoured). ``density_scale``: given, or the voxel edge ``grid_res / grid_scale`` in
        metres when both are, else 1."""
        voxels = _load(voxels_npy)
        sigma = _load(sigma_npy)
        if sigma.ndim != 2 or voxels.ndim != 2 or sigma.shape[0] != voxels.shape[0]:
            raise ANRError(f"sigma must be (n, bands) beside voxels (n, 3), got {sigma.shape} "
                           f"and {voxels.shape}")
        if not -sigma.shape[1] <= band < sigma.shape[1]:
            raise ANRError(f"band {band} of a sigma with {sigma.shape[1]} bands")
        if density_scale is None:
            density_scale = voxel_edge(grid_res, grid_scale) if grid_res is not None else 1.0
        return cls.from_voxels(torch.from_numpy(np.ascontiguousarray(voxels)).to(device),
                               torch.from_numpy(np.ascontiguousarray(sigma[:, band])).to(device),
                               density_scale)

    def light(self, settings: VolumeRenderSettings | None = None,
              skip: bool = True) -> LightVolume:
        """``anr_sparse_volume_light``: the :class:`LightVolume` of this volume under
        ``settings`` (default :func:`global_settings`), ``tau`` (n,) f32 in value order (as
        many bytes again as ``values``). The volume is immutable, so the last one built is
        kept and returned again for settings with the same :func:`light_key`; other settings
        build another. ``skip=False`` switches the brick level off (same values)."""
        settings = global_settings(self) if settings is None else settings
        key = light_key(settings)
        if self._light is not None and self._light[0] == key:
            return self._light[1]
        tau = torch.empty_like(self.values)
        with torch.cuda.device(self.device):
            _lib.call("anr_sparse_volume_light", ctypes.byref(self.desc(skip)), int(skip),
                      settings.params(), _lib.ptr(tau), _lib.stream(self.device))
        self._light = (key, LightVolume(tau, key))
        return self._light[1]

    def sample(self, positions: torch.Tensor, skip: bool = True) -> torch.Tensor:
        """``D`` at (P, 3) f32 box-relative positions (``anr_sparse_volume_sample``): (P,)
        f32. ``skip=False`` looks every corner up instead of asking the brick level first;
        the values are the same."""
        if not positions.is_cuda or positions.device != self.device:
            raise ANRError("SparseVolume.sample needs GPU positions on the volume's device "
                           "(got a CPU tensor or another device)")
        if positions.dim() != 2 or positions.shape[1] != 3 or positions.dtype != torch.float32:
            raise ANRError(f"positions must be (P, 3) float32, got {tuple(positions.shape)} "
                           f"{positions.dtype}")
        positions = positions.contiguous()
        out = torch.empty(positions.shape[0], dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            _lib.call("anr_sparse_volume_sample", ctypes.byref(self.desc(skip)), int(skip),
                      _lib.ptr(positions), positions.shape[0], _lib.ptr(out),
                      _lib.stream(self.device))
        return out


def _load(a) -> np.ndarray:
    if isinstance(a, (str, os.PathLike)):
        return np.load(a, allow_pickle=False)
    if isinstance(a, torch.Tensor):
        return a.detach().cpu().numpy()
    return np.asarray(a)


def voxel_edge(grid_res: float, grid_scale: float | None = None) -> float:
    """The voxel edge in metres, ``grid_res / scale``; ``scale`` defaults to the reference's
    100 / EARTH_RADIUS."""
    if grid_scale is None:
        from .geospatial.spherical import EARTH_RADIUS

        grid_scale = 100 / EARTH_RADIUS
    if not (grid_res > 0 and grid_scale > 0):
        raise ANRError("grid_res and grid_scale must be positive")
    return float(grid_res) / float(grid_scale)


def render_sparse_volume(volume: SparseVolume, cameras: torch.Tensor, width: int = 640,
                         height: int = 480, settings: VolumeRenderSettings | None = None,
                         max_bytes: int = 1 << 28, skip: bool = True,
                         counters: torch.Tensor | None = None, shadows: str = "marched",
                         light: LightVolume | None = None) -> torch.Tensor:
    """(F, height, width, 4) f32 RGBA on the device: ``anr_sparse_volume_render`` of
    ``volume`` from the (F, 12) f32 box-relative ``cameras``; ``settings`` default to
    :func:`global_settings`. Mirrors ``render_volume``: the frames go to the kernel in chunks
    whose output stays under ``max_bytes`` (at least one frame per launch), and frames are
    independent, so the chunking does not change a bit. ``skip=False`` switches the brick
    level off (same output). ``counters``: a zeroed (2,) int64 GPU tensor that receives the
    samples taken inside the box and those of them the brick level answered.

    ``shadows="light_volume"``: ``anr_sparse_volume_render_lit`` with ``light``, by default
    ``volume.light(settings)`` (built once, then kept by the volume); one built for other
    settings raises ANRError. An unknown ``shadows`` raises ValueError."""
    lit = check_shadows(shadows)
    if not isinstance(volume, SparseVolume):
        raise ANRError("render_sparse_volume needs a SparseVolume")
    settings = global_settings(volume) if settings is None else settings
    if not cameras.is_cuda:
        raise ANRError("render_sparse_volume needs GPU tensors (got a CPU tensor)")
    if cameras.dim() != 2 or cameras.shape[1] != 12 or cameras.dtype != torch.float32:
        raise ANRError(f"cameras must be (F, 12) float32, got {tuple(cameras.shape)} "
                       f"{cameras.dtype}")
    if cameras.device != volume.device:
        raise ANRError("volume and cameras must be on one device")
    if counters is not None and (counters.device != volume.device or counters.shape != (2,)
                                 or counters.dtype != torch.int64):
        raise ANRError("counters must be a (2,) int64 tensor on the volume's device")
    cameras = cameras.contiguous()
    F = cameras.shape[0]
    out = torch.empty((F, height, width, 4), dtype=torch.float32, device=volume.device)
    if out.numel() == 0:
        return out
    params, desc = settings.params(), volume.desc(skip)
    chunk = max(1, int(max_bytes) // (height * width * 16))
    if lit:
        light = volume.light(settings, skip) if light is None else light
        light.check(settings, volume.values.shape, volume.device)
        tau = light.tau.contiguous()
    with torch.cuda.device(volume.device):
        for f0 in range(0, F, chunk):
            n = min(chunk, F - f0)
            if lit:
                _lib.call("anr_sparse_volume_render_lit", ctypes.byref(desc), _lib.ptr(tau),
                          int(skip), _lib.ptr(cameras[f0:f0 + n]), n, height, width, params,
                          _lib.ptr(out[f0:f0 + n]), _lib.ptr(counters),
                          _lib.stream(volume.device))
                continue
            _lib.call("anr_sparse_volume_render", ctypes.byref(desc), int(skip),
                      _lib.ptr(cameras[f0:f0 + n]), n, height, width, params,
                      _lib.ptr(out[f0:f0 + n]), _lib.ptr(counters), _lib.stream(volume.device))
    return out


def global_vertical(volume) -> np.ndarray:
    """The local vertical at the data, f64: the grid's origin is the Earth's centre, so it is
    ``normalize(lo + ext / 2)`` in grid coordinates."""
    c = np.asarray(volume.lo, dtype=np.float64) + np.asarray(volume.ext, dtype=np.float64) / 2.0
    norm = float(np.linalg.norm(c))
    if not norm > 0.0:
        raise ANRError("the box is centred on the grid's origin: no local vertical")
    return c / norm


def global_settings(volume, **kw) -> VolumeRenderSettings:
    """``VolumeRenderSettings`` with the light straight up along the local vertical (the
    script's "straight up"); everything else keeps its default or comes from ``kw``."""
    kw.setdefault("light_dir", tuple(global_vertical(volume).tolist()))
    return VolumeRenderSettings(**kw)


def global_orbit_cameras(volume, duration: float = 10.0, frame_rate: int = 60, width: int = 640,
                         height: int = 480, hfov: float = DEFAULT_HFOV,
                         device: torch.device | str | None = None) -> torch.Tensor:
    """The orbit of scripts/make_video.py:155-169 about the local vertical ``n`` through the
    box centre ``c = ext / 2`` (box-relative): ``int(duration * frame_rate)`` frames at
    ``linspace(0, duration, n)``, eye ``c + 1.3 |ext| (cos a e1 + sin a e2) + 0.5 |ext| n``
    with ``e1``, ``e2`` a right-handed pair perpendicular to ``n``, looking at ``c`` with up
    ``n``. The first and the last frame coincide exactly. Returns (frames, 12) f32 on ``device`` (the
    volume's by default); the maths is f64 on the host. ``volume``: anything with ``lo`` and
    ``ext``."""
    n_frames = int(duration * frame_rate)
    if n_frames < 1 or duration <= 0:
        raise ANRError(f"global_orbit_cameras: no frames (duration {duration}, frame rate "
                       f"{frame_rate})")
    ext = np.asarray(volume.ext, dtype=np.float64)
    up = global_vertical(volume)
    # e1: perpendicular to the vertical, from the axis the vertical leans on least
    axis = np.zeros(3)
    axis[int(np.argmin(np.abs(up)))] = 1.0
    e1 = np.cross(up, axis)
    e1 = e1 / np.linalg.norm(e1)
    e2 = np.cross(up, e1)
    centre, norm = ext / 2.0, float(np.linalg.norm(ext))
    ang = 2.0 * np.pi * np.linspace(0.0, duration, n_frames) / duration
    ang[-1] = ang[0]  # one full turn: the same pose, not one a rounding of 2 pi away
    cams = np.stack([
        look_at_camera(centre + 1.3 * norm * (math.cos(a) * e1 + math.sin(a) * e2)
                       + 0.5 * norm * up, centre, up, width, height, hfov)
        for a in ang])
    device = getattr(volume, "device", "cuda") if device is None else device
    return torch.from_numpy(cams.astype(np.float32)).to(device)


def make_global_video(volume, out_dir, video_path=None, sigma=None, band: int = 2,
                      density_scale: float | None = None, grid_res: float | None = None,
                      grid_scale: float | None = None, width: int = 640, height: int = 480,
                      duration: float = 10.0, frame_rate: int = 60,
                      settings: VolumeRenderSettings | None = None,
                      device: torch.device | str = "cuda", max_bytes: int = 1 << 28,
                      shadows: str = "marched", light: LightVolume | None = None) -> dict:
    """The orbit video of a global-grid extract. ``volume``: a :class:`SparseVolume`, or the
    voxels (``voxels.npy`` or an (n, 3) array) with ``sigma`` (``sigma.npy`` or (n, bands)),
    which go through :meth:`SparseVolume.from_files` with ``band``, ``density_scale``,
    ``grid_res`` and ``grid_scale``. One frame per camera of :func:`global_orbit_cameras` is
    written to ``out_dir`` as ``%06d.ppm`` and, with a ``video_path`` and an ``ffmpeg`` binary
    already on PATH, stitched by the script's ffmpeg call. Returns what ``make_video``
    returns, ``"shape"`` being the box extents. ``shadows="light_volume"``: the light volume
    is built once for the whole video (``volume.light``), or ``light`` is taken, if it was
    built for these settings."""
    lit = check_shadows(shadows)
    if not isinstance(volume, SparseVolume):
        if sigma is None:
            raise ANRError("make_global_video: voxels need their sigma")
        volume = SparseVolume.from_files(volume, sigma, band, density_scale, grid_res,
                                         grid_scale, device)
    cameras = global_orbit_cameras(volume, duration, frame_rate, width, height)
    if lit and light is None:
        light = volume.light(settings)
    out_dir = Path(out_dir)
    out_dir.mkdir(parents=True, exist_ok=True)
    frames = []
    chunk = max(1, int(max_bytes) // max(1, height * width * 16))
    for f0 in range(0, cameras.shape[0], chunk):
        rgba = render_sparse_volume(volume, cameras[f0:f0 + chunk], width, height, settings,
                                    max_bytes, shadows=shadows, light=light if lit else None)
        for k, img in enumerate(rgba.cpu().numpy()):
            frames.append(str(out_dir / f"{f0 + k:06d}.ppm"))
            write_ppm(frames[-1], img)
    result = {"frames": frames, "shape": tuple(volume.ext), "video": None}
    return stitch_frames(result, out_dir, video_path, frame_rate, width, height)
