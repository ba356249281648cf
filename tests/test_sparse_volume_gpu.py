"""The sparse volume of a global-grid extract on the GPU (csrc/sparse_volume.hip): its build
against a numpy restatement, its lookup against a float32 trilinear of the densified cube, its
march against anr_volume_render on that cube (bit for bit) and against the f64 yardstick
(tests/volume_checks.py, the tolerance convention of tests/test_volume_gpu.py), and the host
layer up to the orbit frames. Inputs and restatements: tests/sparse_volume_checks.py.
"""

import numpy as np
import pytest
import torch

from tests import sparse_volume_checks as sc
from tests import volume_checks as vc

pytestmark = pytest.mark.gpu


def _t(a, dev):
    return torch.from_numpy(np.array(a)).to(dev)  # a copy: the inputs are read-only


def _volume(dev, voxels, values, scale=1.0):
    from atmonr_amd.sparse_volume import SparseVolume

    return SparseVolume.from_voxels(_t(voxels, dev), _t(values, dev), scale)


def _settings(P: vc.Params):
    from atmonr_amd.video import VolumeRenderSettings

    return VolumeRenderSettings(**{k: getattr(P, k) for k in P.__dataclass_fields__})


def _sparse(dev, vol, cams, H, W, P, **kw):
    from atmonr_amd.sparse_volume import render_sparse_volume

    out = render_sparse_volume(vol, _t(cams, dev), W, H, _settings(P), **kw)
    torch.cuda.synchronize()
    return out


def _dense(dev, cube, cams, H, W, P):
    from atmonr_amd.video import render_volume

    out = render_volume(_t(cube, dev), _t(cams, dev), W, H, _settings(P))
    torch.cuda.synchronize()
    return out


def _parts(vol):
    cells = vol.cells.cpu().numpy().view(np.uint32)
    return cells[:, 0], cells[:, 1].astype(np.int64), vol.values.cpu().numpy(), \
        vol.coarse.cpu().numpy().view(np.uint32)


# ------------------------------------------------------------------ 1. build
def test_build_matches_the_numpy_restatement(dev):
    """Bits, ranks, ordered values and brick bits of the build case (row pitch 96, bits 0, 31,
    32, 63, 64, 69 of one row, a full word, an empty row), from two different shuffles."""
    want = sc.np_build(*sc.build_case(), sc.BUILD_SCALE)
    assert want["lo"] == sc.BUILD_LO and want["ext"] == sc.BUILD_EXT and want["row_pitch"] == 96
    ni, nj, nk = sc.BUILD_EXT
    row = lambda jk: (jk[1] * nj + jk[0]) * 3  # noqa: E731
    assert want["bits"][row(sc.EDGE_ROW):row(sc.EDGE_ROW) + 3].tolist() == \
        [0x80000001, 0x80000001, 0x21]
    assert want["bits"][row(sc.FULL_ROW) + 1] == 0xFFFFFFFF
    assert not want["bits"][row(sc.EMPTY_ROW):row(sc.EMPTY_ROW) + 3].any()
    got = []
    for seed in (1, 2):
        vol = _volume(dev, *sc.shuffled(seed), sc.BUILD_SCALE)
        assert vol.lo == want["lo"] and vol.ext == want["ext"] and vol.row_pitch == 96
        assert len(vol) == want["popcount"] == sc.build_case()[0].shape[0]
        got.append(_parts(vol))
        for g, key in zip(got[-1], ("bits", "rank", "values", "coarse")):
            assert np.array_equal(g, want[key]), (seed, key)
    for a, b in zip(*got):
        assert np.array_equal(a, b)
    # NaN became 0 and the scale went in, in f64 with one rounding
    voxels, values = sc.build_case()
    assert np.isnan(values[17]) and got[0][2][17] == 0.0
    k = 100
    assert got[0][2][k] == np.float32(np.float64(values[k]) * sc.BUILD_SCALE) != values[k]
    n = vol.nbytes
    assert n["cells"] == 8 * 3 * nj * nk and n["values"] == 4 * len(vol)
    assert n["total"] == n["cells"] + n["values"] + n["coarse"]


def test_build_refusals(dev):
    from atmonr_amd._lib import ANRError
    from atmonr_amd.sparse_volume import SparseVolume

    voxels, values = sc.shuffled(1)
    dup_v = np.concatenate([voxels, voxels[5:6]])
    dup_x = np.concatenate([values, values[5:6]])
    with pytest.raises(ANRError, match="duplicate"):
        _volume(dev, dup_v, dup_x)
    with pytest.raises(ANRError, match="n = 0"):
        _volume(dev, voxels[:0], values[:0])
    with pytest.raises(ANRError, match="CPU"):
        SparseVolume.from_voxels(torch.from_numpy(voxels), torch.from_numpy(values))
    with pytest.raises(ANRError, match="CPU"):
        SparseVolume.from_voxels(_t(voxels, dev), torch.from_numpy(values))


# ------------------------------------------------------------------ 2. lookup
def test_lookup_equals_the_f32_trilinear_of_the_densified_cube(dev):
    """All voxel centres, interior points, every face at -1, -0.5, n - 1, n - 0.5 and n, points
    over the pad bits of the rows (i in [ni - 1, row_pitch]: they read 0 and do not wrap into
    the next row), NaN and far-away points; with the brick level and without."""
    voxels, values = sc.shuffled(2)
    vol = _volume(dev, voxels, values, sc.BUILD_SCALE)
    pts = sc.lookup_points()
    want = sc.np_trilinear(sc.densify(voxels, values, sc.BUILD_SCALE), pts)
    ni = sc.BUILD_EXT[0]
    assert (want != 0).mean() > 0.25 and np.all(want[np.floor(pts[:, 0]) >= ni] == 0)
    assert np.all(want[~np.isfinite(pts).all(axis=1)] == 0)
    for skip in (True, False):
        got = vol.sample(_t(pts, dev), skip=skip).cpu().numpy()
        bad = np.flatnonzero(got.view(np.uint32) != want.view(np.uint32))
        assert bad.size == 0, (skip, bad[:5], pts[bad[:5]], got[bad[:5]], want[bad[:5]])
    assert vol.sample(_t(pts[:0], dev)).shape == (0,)


# ------------------------------------------------------------------ 3. render == dense kernel
@pytest.mark.parametrize("name", vc.CASES)
def test_render_equals_the_dense_kernel_half_emptied(dev, name):
    voxels, values, cube, cams, H, W, P = sc.half_case(name)
    vol = _volume(dev, voxels, values)
    assert vol.lo == sc.HALF_LO and vol.ext == vc.SHAPE
    dense = _dense(dev, cube, cams, H, W, P)
    assert float(dense[..., 3].max()) > 0.05
    for skip in (True, False):
        assert torch.equal(_sparse(dev, vol, cams, H, W, P, skip=skip), dense), skip


@pytest.fixture(scope="module")
def shell(dev):
    voxels, values = sc.shell_case()
    perm = np.random.default_rng(4).permutation(voxels.shape[0])
    vol = _volume(dev, voxels[perm], values[perm])
    assert vol.ext == sc.SHELL_EXT and vol.lo == sc.SHELL_LO
    return vol, sc.densify(voxels, values)


@pytest.mark.parametrize("P", [vc.Params(), vc.Params(cutoff=0.0, shadow_step=1.0)],
                         ids=["defaults", "cutoff0_shadow1"])
def test_render_equals_the_dense_kernel_shell(dev, shell, P):
    """Three orbit poses and an eye inside the box, 32 x 24 pixels: brick level on, off, and
    the dense kernel on the densified cube are equal bit for bit, and the brick level answers
    a share of the samples."""
    vol, cube = shell
    cams = sc.shell_cameras()
    H, W = sc.SHELL_H, sc.SHELL_W
    dense = _dense(dev, cube, cams, H, W, P)
    assert float(dense[..., 3].max()) > 0.2 and bool((dense[..., 3] > 0).sum(dim=(1, 2)).min() > 20)
    counters = torch.zeros(2, dtype=torch.int64, device=dev)
    on = _sparse(dev, vol, cams, H, W, P, skip=True, counters=counters)
    off = _sparse(dev, vol, cams, H, W, P, skip=False)
    plain = _sparse(dev, vol, cams, H, W, P, skip=True)
    assert torch.equal(on, dense) and torch.equal(off, dense) and torch.equal(plain, dense)
    samples, skipped = counters.tolist()
    print(f"shell: {skipped} of {samples} samples answered by the brick level "
          f"({skipped / max(1, samples):.1%})")
    assert 0 < skipped < samples
    off_counters = torch.zeros(2, dtype=torch.int64, device=dev)
    _sparse(dev, vol, cams, H, W, P, skip=False, counters=off_counters)
    assert off_counters.tolist() == [samples, 0]


# ------------------------------------------------------------------ 4. render vs the f64 yardstick
@pytest.mark.parametrize("name", vc.CASES)
def test_render_against_the_f64_yardstick(dev, name):
    """Independent of the dense kernel: per channel, on the pixels the yardstick does not
    exclude (at least 98 % of them; tests/test_sparse_volume_cpu.py asserts the share), the
    largest absolute difference to the f64 yardstick is <= max(4 e_arm, 2^-20 max|yardstick|)."""
    voxels, values, cube, cams, H, W, P = sc.half_case(name)
    got = _sparse(dev, _volume(dev, voxels, values), cams, H, W, P).cpu().numpy()
    assert got.shape == (cams.shape[0], H, W, 4) and np.isfinite(got).all()
    keep = sc.half_compared(name)
    e_gpu, e_arm, bound = sc.half_errors(name, got)
    print(f"{name}: e_gpu {e_gpu.tolist()} e_arm {e_arm.tolist()} bound {bound.tolist()} "
          f"compared {int(keep.sum())} of {keep.size} pixels")
    assert keep.mean() >= 0.98
    assert np.all(e_gpu <= bound), (name, e_gpu, bound)
    miss = sc.half_reference(name)[0]["flags"][..., 3]
    assert np.all(got[miss] == 0.0)


# ------------------------------------------------------------------ 5. frames and chunking
def test_frames_are_independent(dev):
    """Three cameras in one launch equal three single-camera launches bit for bit, and so does
    a render_sparse_volume call forced to cut the frames into chunks."""
    voxels, values, _, cams, H, W, P = sc.half_case("cutoff")
    vol = _volume(dev, voxels, values)
    whole = _sparse(dev, vol, cams, H, W, P)
    for f in range(cams.shape[0]):
        assert torch.equal(_sparse(dev, vol, cams[f:f + 1], H, W, P)[0], whole[f]), f
    for budget in (H * W * 16, 1, 2 * H * W * 16):
        assert torch.equal(_sparse(dev, vol, cams, H, W, P, max_bytes=budget), whole)
    assert _sparse(dev, vol, cams[:0], H, W, P).shape == (0, H, W, 4)


# ------------------------------------------------------------------ 6. host layer
def test_make_global_video_writes_the_orbit_frames(dev, shell, tmp_path):
    from atmonr_amd.sparse_volume import (SparseVolume, global_orbit_cameras, global_settings,
                                          global_vertical, make_global_video,
                                          render_sparse_volume)
    from atmonr_amd.video import read_ppm, write_ppm

    vol, _ = shell
    res = make_global_video(vol, tmp_path / "frames", None, width=32, height=24, duration=1.0,
                            frame_rate=4)
    assert res["shape"] == sc.SHELL_EXT and res["video"] is None and "frames stay" in res["ffmpeg"]
    names = sorted(p.name for p in (tmp_path / "frames").iterdir())
    assert names == ["000000.ppm", "000001.ppm", "000002.ppm", "000003.ppm"]
    head = b"P6\n32 24\n255\n"
    for p in res["frames"]:
        raw = open(p, "rb").read()
        assert raw.startswith(head) and len(raw) == len(head) + 32 * 24 * 3
    cams = global_orbit_cameras(vol, 1.0, 4, 32, 24)
    assert cams.device == vol.device and cams.shape == (4, 12)
    assert global_settings(vol).light_dir == tuple(global_vertical(vol).tolist())
    first = render_sparse_volume(vol, cams[:1], 32, 24)[0]
    write_ppm(tmp_path / "first.ppm", first)
    assert open(tmp_path / "first.ppm", "rb").read() == open(res["frames"][0], "rb").read()
    assert read_ppm(res["frames"][0]).max() > 20  # the shell is lit, not a black frame
    # the same frames from the two files an extract dumps, band 1 of two
    voxels, values = sc.shell_case()
    np.save(tmp_path / "voxels.npy", voxels)
    np.save(tmp_path / "sigma.npy", np.stack([np.zeros_like(values), values], axis=1))
    again = make_global_video(tmp_path / "voxels.npy", tmp_path / "again", None,
                              sigma=tmp_path / "sigma.npy", band=1, width=32, height=24,
                              duration=1.0, frame_rate=4, device=dev)
    for a, b in zip(res["frames"], again["frames"]):
        assert open(a, "rb").read() == open(b, "rb").read()
    from atmonr_amd._lib import ANRError

    with pytest.raises(ANRError, match="band"):
        SparseVolume.from_files(tmp_path / "voxels.npy", tmp_path / "sigma.npy", band=2, device=dev)


def test_global_grid_dataset_volume(dev):
    """GlobalGridExtractDataset.volume on the tiny synthetic scene of
    tests/test_globalgrid_gpu.py: as many bits as the dataset has voxels, and the lookup at a
    voxel's box-relative position returns its value times the voxel edge."""
    from atmonr_amd._lib import ANRError
    from atmonr_amd.datasets.synthetic import SyntheticHARP2Dataset
    from atmonr_amd.extract import GlobalGridExtractDataset
    from atmonr_amd.geospatial.spherical import EARTH_RADIUS

    scene = SyntheticHARP2Dataset(n_views=8, img_size=16, device=dev, seed=0)
    ds = GlobalGridExtractDataset(scene, 100 / EARTH_RADIUS, 0.025, 12, 0.05)
    n = len(ds)
    gen = torch.Generator(device="cpu").manual_seed(1)
    sigma = (torch.rand((n, 3), generator=gen) * 2e-4).to(dev)
    vol = ds.volume(sigma)
    bits = vol.cells.cpu().numpy().view(np.uint32)[:, 0]
    assert len(vol) == n == sum(bin(int(w)).count("1") for w in bits[bits != 0])
    assert vol.lo == tuple(ds.voxels.amin(dim=0).tolist())
    assert vol.density_scale == 0.025 / (100 / EARTH_RADIUS)
    pos = (ds.voxels - torch.tensor(vol.lo, device=dev)).float()
    want = (sigma[:, 2].double() * vol.density_scale).float()
    assert torch.equal(vol.sample(pos), want)
    assert torch.equal(vol.values, want)  # the dataset's voxels are in bitmap order already
    assert torch.equal(ds.volume(sigma, band=0).sample(pos),
                       (sigma[:, 0].double() * vol.density_scale).float())
    with pytest.raises(ANRError, match="band"):
        ds.volume(sigma, band=3)
    with pytest.raises(ANRError, match="bands"):
        ds.volume(sigma[:-1])
