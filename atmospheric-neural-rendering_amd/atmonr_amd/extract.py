"""Volume extraction — the loop of scripts/extract.py:180-211 over the L1C-style grid of
datasets/harp2_extract.py:71-187.

``GridExtractDataset`` builds the query points exactly as ``HARP2L1CExtractDataset``:
``sample_alt = arange(min_alt, max_alt + alt_step / 2, alt_step)`` (f32, the torch default
dtype), every horizontal grid cell repeated over the altitudes, converted to WGS-84
Cartesian in f64 (``horizontal_to_cartesian``). The horizontal grid is the dataset's
pixel lat/lon (the L1C grid needs the NASA download, absent offline) or any (H, W) lat/lon
the caller passes (voxel-grid mode).

``extract_volume`` runs the reference loop: batches of ``batch_size`` columns
(``batch_size · n_alt`` points, unshuffled), ``pts = (xyz - offset) / scale`` in f64,
``sigma[idx] = pipeline.extract(pts) / scale``. On MI355X the points stay in HBM, the
f64 preprocessor runs as one kernel (anr_preprocess_points_f64) and the hash encoder +
density MLP as the same kernels training uses; the host only slices index ranges.
``dump`` writes an .npz with the reference's netCDF variables (netCDF4 is not installed).

``GlobalGridExtractDataset`` is the global voxel grid of ``HARP2GlobalGridExtractDataset``
(harp2_extract.py:794-946, ``--coord-mode globalgrid``): the voxels that the training rays
pass through in a stretched spherical-Earth frame, found by an exact traversal on the GPU
(csrc/voxels.hip). It needs nothing but the training rays. ``get_extract_dataset`` maps the
script's coordinate modes to the classes here.
"""

from __future__ import annotations

import inspect
from pathlib import Path

import numpy as np
import torch

from .batch_loader import BatchLoader
from .geospatial.spherical import (spherical_to_wgs84, stretch_above_sea_level,
                                   wgs_84_to_spherical)
from .geospatial.wgs_84 import cartesian_to_horizontal, horizontal_to_cartesian


class GridExtractDataset:
    def __init__(self, dataset, alt_step: float = 250.0, min_alt: float | None = None,
                 max_alt: float | None = None, lat: torch.Tensor | None = None,
                 lon: torch.Tensor | None = None) -> None:
        self.dataset = dataset
        self.device = dataset.device
        self.alt_step = alt_step
        self.min_alt = 0 if min_alt is None else min_alt
        self.max_alt = dataset.config["ray_origin_height"] if max_alt is None else max_alt
        self.sample_alt = torch.arange(self.min_alt, self.max_alt + self.alt_step / 2,
                                       self.alt_step).to(self.device)
        if lat is None:
            H, W = dataset.img_shp
            lat = dataset.lat[:, 0].view(H, W)
            lon = dataset.lon[:, 0].view(H, W)
        self.shp = tuple(lat.shape)
        A = self.sample_alt.shape[0]
        self.lat = lat[:, :, None].repeat(1, 1, A).to(self.device)
        self.lon = lon[:, :, None].repeat(1, 1, A).to(self.device)
        alt = self.sample_alt[None, None].repeat(self.lat.shape[0], self.lat.shape[1], 1)
        xyz = torch.stack(list(horizontal_to_cartesian(
            self.lat.double(), self.lon.double(), alt.double())), dim=-1)
        self.xyz = xyz.view(-1, 3)
        self.idx = torch.arange(self.xyz.shape[0], device=self.device, dtype=torch.int64)

    def __len__(self) -> int:
        return int(self.xyz.shape[0])

    def __getbatch__(self, idx: torch.Tensor) -> dict[str, torch.Tensor]:
        return {"xyz": self.xyz[idx], "idx": self.idx[idx]}

    __getitem__ = __getbatch__

    def dump(self, path: Path | str, sigma: torch.Tensor) -> None:
        """Variables of _extract_to_netCDF (harp2_extract.py:429-596) as an .npz."""
        A = self.sample_alt.shape[0]
        np.savez(path,
                 extinction=sigma.view(*self.shp, A, -1).cpu().numpy(),
                 latitude=self.lat[:, :, 0].cpu().numpy(),
                 longitude=self.lon[:, :, 0].cpu().numpy(),
                 sample_alt=self.sample_alt.cpu().numpy(),
                 xyz=self.xyz.view(*self.shp, A, 3).cpu().numpy())


def voxel_centers(voxels: torch.Tensor, grid_res: float, scale: float) -> torch.Tensor:
    """Voxel indices (n, 3) -> centres (n, 3) f64 in the (stretched) spherical frame, metres
    (harp2_extract.py:872)."""
    return (voxels.double() + 0.5) * (grid_res / scale)


def crop_and_cull(voxels: torch.Tensor, grid_res: float, scale: float, vstretch: float,
                  lon_crop: float, ray_origin_height: float):
    """harp2_extract.py:871-902 on voxel indices (n, 3), on any device: returns (``xyz``
    (m, 3) f64 WGS-84 Cartesian voxel centres, ``voxels`` (m, 3), ``keep`` (n,) bool), the
    kept rows in their input order.

    * Crop: within each z-layer (one value of k), with the spherical longitude
      ``atan2(y, x)`` of the stretched centres, keep ``min + c * range < lon < max - c *
      range`` for c = ``lon_crop``. Strict, so a layer of one longitude is dropped whole. The
      reference's loop over the layers is a pair of per-layer ``amin`` / ``amax`` reductions.
    * Cull: un-stretch the centres with ``1 / vstretch``, convert to WGS-84 and drop those
      whose ellipsoidal height is ``<= 0`` or ``> ray_origin_height`` (the reference's
      ``alt <= 0 + alt > h`` is a chained comparison that cannot run on a tensor)."""
    centers = voxel_centers(voxels, grid_res, scale)
    lon = torch.atan2(centers[:, 1], centers[:, 0])
    if voxels.shape[0]:
        layer = (voxels[:, 2] - voxels[:, 2].amin()).long()
        n_layers = int(layer.amax().item()) + 1
    else:
        layer, n_layers = voxels[:, 2].long(), 0
    inf = torch.full((n_layers,), float("inf"), dtype=lon.dtype, device=lon.device)
    lon_min = inf.scatter_reduce(0, layer, lon, "amin")
    lon_max = (-inf).scatter_reduce(0, layer, lon, "amax")
    lon_range = lon_max - lon_min
    keep = (lon > (lon_min + lon_crop * lon_range)[layer]) & \
        (lon < (lon_max - lon_crop * lon_range)[layer])
    xyz = spherical_to_wgs84(stretch_above_sea_level(centers, 1 / vstretch))
    _, _, alt = cartesian_to_horizontal(xyz[:, 0], xyz[:, 1], xyz[:, 2])
    keep &= ~((alt <= 0) | (alt > ray_origin_height))
    return xyz[keep], voxels[keep], keep


class GlobalGridExtractDataset:
    """``HARP2GlobalGridExtractDataset`` (harp2_extract.py:794-946): the voxels of a global
    grid (spherical-Earth frame times ``scale``, voxel edge ``grid_res``) that the dataset's
    rays pass through, with the atmosphere stretched by ``vstretch`` so that a global view
    shows its vertical structure. Stage by stage (harp2_extract.py:819-903):

    1. ray origin and destination in metres (``ray_origin_norm * scale + offset``, plus
       ``ray_dir * ray_len_norm * scale``), f64;
    2. to the spherical frame; 3. stretch above sea level; 4. times ``scale / grid_res``;
    5. exact traversal of ``chunk`` rays at a time into one bitmap; 6. its compaction;
    7. voxel centres ``(v + 0.5) * grid_res / scale``; 8. per z-layer longitude crop;
    9. un-stretch with ``1 / vstretch``; 10. back to WGS-84; 11. cull by altitude
    (7-11: :func:`crop_and_cull`).

    ``xyz`` (n, 3) f64 are the WGS-84 Cartesian query points, ``voxels`` (n, 3) int32 their
    grid indices, ``idx`` arange(n). ``scale`` is the grid's own (the reference's default is
    100 / EARTH_RADIUS), not the dataset's normalisation.

    Deliberate differences from the reference's letter:

    * the traversal is exact in f64; the reference accumulates ``tmax += tdelta`` in f32 and
      can leave the true path where the coordinates are large;
    * indices are int32, not int16 (a grid of the reference's default size reaches +-4100,
      finer ones pass int16);
    * the cull is ``(alt <= 0) | (alt > ray_origin_height)``: the reference's line 899 is a
      chained comparison of tensors, which raises;
    * ``voxels`` are the traversal's own indices; the reference recovers them from the centres
      by truncation toward zero (line 886), which agrees for non-negative coordinates only;
    * the voxel order is the bitmap's (k slowest, i fastest), whatever the ray order; the
      reference's is that of ``torch.unique(sorted=False)`` within each layer;
    * ``xyz`` stays f64 (the reference's centres pass through f32).
    """

    def __init__(self, dataset, scale: float, grid_res: float, vstretch: float | None = None,
                 lon_crop: float = 0.05, chunk: int = 1 << 22,
                 max_bitmap_bytes: int | None = None) -> None:
        from .graphics_utils import DEFAULT_MAX_BITMAP_BYTES, VoxelBitmap

        if vstretch is None:
            vstretch = 1
        if not vstretch >= 1:
            raise ValueError(f"vstretch {vstretch} must be >= 1")
        if not (scale > 0 and grid_res > 0 and chunk >= 1):
            raise ValueError("scale, grid_res and chunk must be positive")
        self.dataset = dataset
        self.device = dataset.device
        self.scale, self.grid_res, self.vstretch = float(scale), float(grid_res), vstretch
        self.lon_crop = lon_crop
        n_rays = len(dataset)
        spans = [(s, min(n_rays, s + chunk)) for s in range(0, n_rays, chunk)]
        lo = hi = None
        for s, e in spans:
            box = VoxelBitmap.bounds(*self._ray_segments(s, e))
            if box is not None:
                lo = box[0] if lo is None else [min(a, b) for a, b in zip(lo, box[0])]
                hi = box[1] if hi is None else [max(a, b) for a, b in zip(hi, box[1])]
        if lo is None:
            raise ValueError("the dataset has no ray with finite endpoints")
        bitmap = VoxelBitmap(lo, hi, self.device, DEFAULT_MAX_BITMAP_BYTES
                             if max_bitmap_bytes is None else max_bitmap_bytes)
        for s, e in spans:
            bitmap.add(*self._ray_segments(s, e))
        self.traversed = bitmap.voxels()  # before the crop and the cull
        self.xyz, self.voxels, _ = crop_and_cull(
            self.traversed, self.grid_res, self.scale, self.vstretch, self.lon_crop,
            dataset.config["ray_origin_height"])
        self.idx = torch.arange(self.xyz.shape[0], device=self.device, dtype=torch.int64)

    def _ray_segments(self, s: int, e: int):
        """Stages 1-4 for rays [s, e): start and end in continuous voxel coordinates, f64."""
        ds = self.dataset
        offset = torch.as_tensor(ds.offset, dtype=torch.float64, device=self.device)
        origin = ds.ray_origin_norm[s:e].double() * ds.scale + offset
        dest = origin + ds.ray_dir[s:e].double() * (ds.ray_len_norm[s:e].double() * ds.scale)[:, None]
        k = self.scale / self.grid_res
        return tuple(stretch_above_sea_level(wgs_84_to_spherical(p), self.vstretch) * k
                     for p in (origin, dest))

    def __len__(self) -> int:
        return int(self.xyz.shape[0])

    def __getbatch__(self, idx: torch.Tensor) -> dict[str, torch.Tensor]:
        return {"xyz": self.xyz[idx], "idx": self.idx[idx]}

    __getitem__ = __getbatch__

    def volume(self, sigma: torch.Tensor, band: int = 2):
        """The :class:`~atmonr_amd.sparse_volume.SparseVolume` of this grid's voxels with band
        ``band`` of ``sigma`` (n, bands), as ``extract_volume`` returns it: what
        ``make_global_video`` renders. The extinction (1/m) is multiplied by the voxel edge in
        metres, ``grid_res / scale``, so the density is optical depth per voxel edge."""
        from ._lib import ANRError
        from .sparse_volume import SparseVolume

        if sigma.dim() != 2 or sigma.shape[0] != len(self):
            raise ANRError(f"sigma must be ({len(self)}, bands), got {tuple(sigma.shape)}")
        if not -sigma.shape[1] <= band < sigma.shape[1]:
            raise ANRError(f"band {band} of a sigma with {sigma.shape[1]} bands")
        return SparseVolume.from_voxels(self.voxels, sigma[:, band].to(self.device),
                                        self.grid_res / self.scale)

    def dump(self, path: Path | str, sigma: torch.Tensor) -> None:
        """The reference's output without the OpenVDB bindings (harp2_extract.py:919-934):
        ``voxels.npy`` and ``sigma.npy`` beside ``path`` (the reference writes them into the
        working directory). FileExistsError when either exists."""
        folder = Path(path).parent
        voxel_path, sigma_path = folder / "voxels.npy", folder / "sigma.npy"
        for f in (voxel_path, sigma_path):
            if f.exists():
                raise FileExistsError(str(f))
        np.save(voxel_path, self.voxels.detach().cpu().numpy(), allow_pickle=False)
        np.save(sigma_path, sigma.detach().cpu().numpy(), allow_pickle=False)


def get_extract_dataset(coord_mode: str, dataset, **kw):
    """scripts/extract.py:150-177: the extract dataset of a ``--coord-mode``. ``l1c`` and
    ``voxelgrid`` are the :class:`GridExtractDataset` (the dataset's own pixel grid, or the
    ``lat`` / ``lon`` passed), ``globalgrid`` the :class:`GlobalGridExtractDataset`;
    ``earthcare`` needs an EarthCARE file and is not built."""
    if coord_mode in ("l1c", "voxelgrid"):
        return GridExtractDataset(dataset, **kw)
    if coord_mode == "globalgrid":
        return GlobalGridExtractDataset(dataset, **kw)
    if coord_mode == "earthcare":
        raise NotImplementedError("coord_mode 'earthcare' reads an EarthCARE file: not built")
    raise ValueError(f"unknown coord_mode {coord_mode!r}")


def _extract(pipeline, pts, run_length):
    """pipeline.extract with the column run length when the pipeline takes the hint (the
    batches are whole columns of ``run_length`` altitudes)."""
    if "run_length" in inspect.signature(pipeline.extract).parameters:
        return pipeline.extract(pts, run_length=run_length)
    return pipeline.extract(pts)


def extract_volume(pipeline, dataset, extract_ds, batch_size: int = 32768,
                   num_bands: int = 1) -> torch.Tensor:
    """scripts/extract.py:183-209: extinction (n_points, num_bands) in 1/m. A dataset of
    columns (``sample_alt``) is read ``batch_size`` columns at a time; one without, such as
    the global grid's voxels, ``batch_size`` points at a time with no run-length hint."""
    columns = getattr(extract_ds, "sample_alt", None)
    A = int(columns.shape[0]) if columns is not None else 0
    loader = BatchLoader(extract_ds, batch_size=batch_size * max(A, 1), shuffle=False)
    sigma = torch.zeros((len(extract_ds), num_bands), device=extract_ds.device)
    offset = torch.as_tensor(dataset.offset, dtype=torch.float64, device=extract_ds.device)
    with torch.no_grad():
        for batch in loader:
            pts = (batch["xyz"] - offset) / dataset.scale
            sigma[batch["idx"]] = _extract(pipeline, pts, A).to(dtype=sigma.dtype) / dataset.scale
    return sigma
