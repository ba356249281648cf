"""GlobalGridExtractDataset and extract_volume over it, on the GPU: the 8-view 16 x 16
synthetic scene in the reference's default grid (scale 100 / EARTH_RADIUS, grid_res 0.025: a
voxel edge of 1,594 m in the stretched frame), vstretch 12, lon_crop 0.05."""

import pytest
import torch

import __graft_entry__ as ge

pytestmark = pytest.mark.gpu

RES, VSTRETCH, CROP = 0.025, 12, 0.05


@pytest.fixture(scope="module")
def scene(dev):
    from atmonr_amd.datasets.synthetic import SyntheticHARP2Dataset

    return SyntheticHARP2Dataset(n_views=8, img_size=16, device=dev, seed=0)


@pytest.fixture(scope="module")
def grid(scene):
    from atmonr_amd.extract import get_extract_dataset
    from atmonr_amd.geospatial.spherical import EARTH_RADIUS

    return get_extract_dataset("globalgrid", scene, scale=100 / EARTH_RADIUS, grid_res=RES,
                               vstretch=VSTRETCH, lon_crop=CROP, chunk=600)


def _key(v):
    v = v.to(torch.int64)
    off = v.amin(dim=0)
    ext = v.amax(dim=0) - off + 1
    r = v - off
    return (r[:, 2] * ext[1] + r[:, 1]) * ext[0] + r[:, 0]


def test_global_grid_dataset(scene, grid, dev):
    """2,048 rays walk 104,665 voxels, of which 91,745 survive the crop and the cull (an
    MI355X run; the test prints its own counts). With vstretch 1 the rays walk about 30 % as
    many."""
    from atmonr_amd.extract import GlobalGridExtractDataset, crop_and_cull, voxel_centers
    from atmonr_amd.geospatial import spherical as sph
    from atmonr_amd.geospatial.wgs_84 import cartesian_to_horizontal

    roh = scene.config["ray_origin_height"]
    n = len(grid)
    print(f"global grid: {grid.traversed.shape[0]} traversed, {n} kept")
    assert 1e3 <= n <= 2e5
    assert grid.xyz.shape == (n, 3) and grid.xyz.dtype == torch.float64
    assert grid.voxels.shape == (n, 3) and grid.voxels.dtype == torch.int32
    assert torch.equal(grid.idx, torch.arange(n, device=dev))
    assert grid.xyz.device == grid.voxels.device == grid.idx.device and grid.xyz.is_cuda
    # unique, and sorted in bitmap order (k slowest, i fastest)
    for v in (grid.traversed, grid.voxels):
        key = _key(v)
        assert bool((key[1:] > key[:-1]).all())
    # every centre's altitude after the un-stretch lies in (0, ray_origin_height]
    c = voxel_centers(grid.voxels, RES, grid.scale)
    xyz = sph.spherical_to_wgs84(sph.stretch_above_sea_level(c, 1 / VSTRETCH))
    assert torch.equal(xyz, grid.xyz)
    alt = cartesian_to_horizontal(xyz[:, 0], xyz[:, 1], xyz[:, 2])[2]
    assert bool((alt > 0).all()) and bool((alt <= roh).all())
    # the kept set is the CPU crop and cull of the traversal's own output
    cx, cv, keep = crop_and_cull(grid.traversed.cpu(), RES, grid.scale, VSTRETCH, CROP, roh)
    assert 0 < int(keep.sum()) < keep.shape[0]
    assert torch.equal(cv, grid.voxels.cpu())
    assert float((cx - grid.xyz.cpu()).abs().max()) <= 1e-6  # CPU and device f64 libm, metres
    # __getbatch__, and the chunking of the rays does not matter
    b = grid.__getbatch__(torch.tensor([5, 0, n - 1], device=dev))
    assert torch.equal(b["xyz"], grid.xyz[[5, 0, n - 1]]) and b["idx"].tolist() == [5, 0, n - 1]
    whole = GlobalGridExtractDataset(scene, grid.scale, RES, VSTRETCH, CROP)
    assert torch.equal(whole.traversed, grid.traversed) and torch.equal(whole.voxels, grid.voxels)
    # without the stretch: a different, smaller set
    flat = GlobalGridExtractDataset(scene, grid.scale, RES, None, CROP)
    assert flat.vstretch == 1 and 0 < len(flat) < n
    assert flat.traversed.shape[0] < grid.traversed.shape[0]
    both = torch.cat([flat.traversed, grid.traversed]).unique(dim=0).shape[0]
    assert both > grid.traversed.shape[0]  # not a subset either
    with pytest.raises(ValueError, match="max_bitmap_bytes"):
        GlobalGridExtractDataset(scene, grid.scale, RES, VSTRETCH, CROP, max_bitmap_bytes=4096)
    with pytest.raises(ValueError, match="vstretch"):
        GlobalGridExtractDataset(scene, grid.scale, RES, 0.5)


def test_extract_volume_over_the_global_grid(scene, grid, dev):
    from atmonr_amd.extract import extract_volume
    from atmonr_amd.pipelines.instant_ngp import InstantNGPPipeline

    p = InstantNGPPipeline(ge._ingp_config(64), scene, seed=5)
    p.send_tensors_to(dev)
    p.eval()
    n = len(grid)
    sigma = extract_volume(p, scene, grid, batch_size=1000)
    assert sigma.shape == (n, 1)
    assert bool(torch.isfinite(sigma).all()) and bool((sigma >= 0).all())
    assert torch.equal(sigma, extract_volume(p, scene, grid, batch_size=32768))
    off = torch.as_tensor(scene.offset, dtype=torch.float64, device=dev)
    direct = p.extract((grid.xyz - off) / scene.scale).float() / scene.scale
    assert torch.equal(sigma, direct)
