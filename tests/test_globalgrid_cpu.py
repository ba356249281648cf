"""The global-grid extract's parts that need no GPU: the spherical-frame helpers against the
reference's outputs (tests/golden/voxel_traversal.npz), the crop and cull on a hand-made
voxel set, the argument checks of the voxel entry points, the dataset factory and ``dump``."""

import ctypes
import math

import numpy as np
import pytest
import torch

from tests.conftest import golden

FAKE = 0x10000  # non-null, never dereferenced: every call here is answered by validation
OK, INVALID = 0, -1


# ------------------------------------------------------------------ spherical helpers
@pytest.fixture(scope="module")
def gold():
    return golden("voxel_traversal.npz")


def _points(gold, name):
    pts = torch.from_numpy(gold["points_f64"])
    return pts.float() if name == "f32" else pts


def _calls():
    from atmonr_amd.geospatial import spherical as sph

    return {"to_spherical": sph.wgs_84_to_spherical, "to_wgs84": sph.spherical_to_wgs84,
            "stretch_12": lambda p: sph.stretch_above_sea_level(p, 12),
            "stretch_inv12": lambda p: sph.stretch_above_sea_level(p, 1 / 12)}


def test_constants_and_fixture(gold):
    from atmonr_amd.geospatial import spherical as sph

    assert sph.EARTH_RADIUS == float(gold["earth_radius"]) == 6.378e6
    pts = _points(gold, "f64")
    r = torch.linalg.norm(pts, dim=-1)
    assert pts.shape == (4096, 3) and float((r - sph.EARTH_RADIUS).abs().max()) <= 30e3
    assert 1000 < int((r > sph.EARTH_RADIUS).sum()) < 3096  # both sides of the sphere


@pytest.mark.parametrize("fn", ["to_spherical", "to_wgs84", "stretch_12", "stretch_inv12"])
def test_helpers_f64_exact(gold, fn):
    pts = _points(gold, "f64")
    keep = pts.clone()
    out = _calls()[fn](pts)
    assert out.dtype == torch.float64 and torch.equal(pts, keep)  # out of place
    assert torch.equal(out, torch.from_numpy(gold[f"{fn}_f64"]))


@pytest.mark.parametrize("fn", ["to_spherical", "to_wgs84", "stretch_12", "stretch_inv12"])
def test_helpers_f32_within_one_ulp(gold, fn):
    pts = _points(gold, "f32")
    keep = pts.clone()
    out = _calls()[fn](pts)
    assert out.dtype == torch.float32 and torch.equal(pts, keep)
    want = torch.from_numpy(gold[f"{fn}_f32"])
    ulp = torch.from_numpy(np.spacing(np.abs(want.numpy())))
    assert bool(((out - want).abs() <= ulp).all())


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_round_trip_identity_and_below_the_sphere(gold, dtype):
    from atmonr_amd.geospatial import spherical as sph

    pts = _points(gold, "f64").to(dtype)
    eps = torch.finfo(dtype).eps
    back = sph.spherical_to_wgs84(sph.wgs_84_to_spherical(pts))
    assert float((back - pts).abs().max()) <= 4 * eps * 6.41e6
    assert torch.equal(sph.stretch_above_sea_level(pts, 1), pts)  # stretch 1: the identity
    r = torch.linalg.norm(pts, dim=-1)
    below = r <= sph.EARTH_RADIUS
    for s in (12, 1 / 12):
        out = sph.stretch_above_sea_level(pts, s)
        assert torch.equal(out[below], pts[below])  # at or below the sphere: untouched
        h = torch.linalg.norm(out, dim=-1)[~below] - sph.EARTH_RADIUS
        assert torch.allclose(h, (r[~below] - sph.EARTH_RADIUS) * s, rtol=0,
                              atol=8 * eps * 6.8e6)
    # 1 / 12 undoes 12
    there = sph.stretch_above_sea_level(sph.stretch_above_sea_level(pts, 12), 1 / 12)
    assert float((there - pts).abs().max()) <= 16 * eps * 6.8e6
    # a point exactly on the sphere, and any leading shape
    on = torch.tensor([[[sph.EARTH_RADIUS, 0.0, 0.0]]], dtype=dtype)
    assert torch.equal(sph.stretch_above_sea_level(on, 12), on)
    assert sph.stretch_above_sea_level(pts.view(64, 64, 3), 12).shape == (64, 64, 3)


# ------------------------------------------------------------------ crop and cull
SCALE, RES, VSTRETCH, ROH = 100 / 6.378e6, 0.025, 12.0, 20000.0
EDGE = RES / SCALE  # voxel edge in the stretched frame, metres (1594.5)


def _hand_made_voxels():
    """Three z-layers near (R, 0, 0): k = 0 with i at four radii (below the surface, low,
    high, above ray_origin_height) times 21 longitudes j; k = 1 with 11 longitudes at one
    radius; k = 2 with a single voxel (longitude range 0)."""
    i_surf = int(6.378e6 // EDGE)  # the voxel that contains the sphere's surface at y = z = 0
    rows = []
    for i in (i_surf - 2, i_surf + 3, i_surf + 100, i_surf + 200):
        rows += [(i, j, 0) for j in range(-10, 11)]
    rows += [(i_surf + 50, j, 1) for j in range(0, 11)]
    rows += [(i_surf + 50, 3, 2)]
    return torch.tensor(rows, dtype=torch.int32), i_surf


def _altitudes(voxels):
    from atmonr_amd.extract import voxel_centers
    from atmonr_amd.geospatial import spherical as sph
    from atmonr_amd.geospatial.wgs_84 import cartesian_to_horizontal

    c = voxel_centers(voxels, RES, SCALE)
    xyz = sph.spherical_to_wgs84(sph.stretch_above_sea_level(c, 1 / VSTRETCH))
    return xyz, cartesian_to_horizontal(xyz[:, 0], xyz[:, 1], xyz[:, 2])[2]


def test_crop_and_cull_on_three_layers():
    from atmonr_amd.extract import crop_and_cull, voxel_centers

    vox, i_surf = _hand_made_voxels()
    c = 0.05
    xyz, kept, keep = crop_and_cull(vox, RES, SCALE, VSTRETCH, c, ROH)
    assert xyz.dtype == torch.float64 and kept.dtype == torch.int32
    assert torch.equal(kept, vox[keep]) and xyz.shape == (int(keep.sum()), 3)
    centers = voxel_centers(vox, RES, SCALE)
    assert torch.equal(centers, (vox.double() + 0.5) * EDGE)
    lon = torch.atan2(centers[:, 1], centers[:, 0])
    all_xyz, alt = _altitudes(vox)
    assert torch.equal(xyz, all_xyz[keep])
    # the hand-made radii do what they were made for (stretched height / 12, then WGS-84)
    by_i = {int(i): alt[(vox[:, 0] == i) & (vox[:, 2] == 0)] for i in vox[:, 0].unique()}
    assert bool((by_i[i_surf - 2] <= 0).all()) and bool((by_i[i_surf + 200] > ROH).all())
    assert bool(((by_i[i_surf + 3] > 0) & (by_i[i_surf + 3] <= ROH)).all())
    for k in (0, 1, 2):
        layer = vox[:, 2] == k
        lo, hi = lon[layer].min(), lon[layer].max()
        inside = (lon > lo + c * (hi - lo)) & (lon < hi - c * (hi - lo)) & layer
        want = inside & (alt > 0) & (alt <= ROH)
        assert torch.equal(keep[layer], want[layer]), k
        # kept longitudes lie strictly inside the cropped range of their own layer
        assert bool((lon[keep & layer] > lo + c * (hi - lo)).all())
        assert bool((lon[keep & layer] < hi - c * (hi - lo)).all())
    # layer 0's range comes from its outermost voxels at the smallest radius, even though
    # those are below the surface: the crop sees every traversed voxel, as the reference's
    assert int(keep[vox[:, 2] == 0].sum()) > 0 and int(keep[vox[:, 2] == 1].sum()) == 9
    assert not bool(keep[vox[:, 2] == 2].any())  # one voxel: range 0, strict inequalities
    assert not bool(keep[alt <= 0].any()) and not bool(keep[alt > ROH].any())
    # the rows keep their input order, and an empty set stays empty
    perm = torch.randperm(vox.shape[0], generator=torch.Generator().manual_seed(1))
    assert torch.equal(crop_and_cull(vox[perm], RES, SCALE, VSTRETCH, c, ROH)[1], vox[perm][keep[perm]])
    e = crop_and_cull(vox[:0], RES, SCALE, VSTRETCH, c, ROH)
    assert e[0].shape == (0, 3) and e[1].shape == (0, 3) and e[2].shape == (0,)


def test_crop_zero_keeps_all_but_the_extremes():
    from atmonr_amd.extract import crop_and_cull

    vox, _ = _hand_made_voxels()
    layer1 = vox[vox[:, 2] == 1]
    _, kept, _ = crop_and_cull(layer1, RES, SCALE, VSTRETCH, 0.0, ROH)
    assert kept[:, 1].tolist() == list(range(1, 10))


# ------------------------------------------------------------------ entry-point arguments
def _L():
    from atmonr_amd import _lib

    return _lib, _lib.load()


def _traverse(lib, **over):
    p = dict(u=FAKE, end=FAKE, R=64, i0=-5, j0=-5, k0=-5, ni=40, nj=10, nk=10, pitch=64,
             bitmap=FAKE, counters=FAKE, shortcut=1)
    assert set(over) <= set(p)
    p.update(over)
    rc = lib.anr_voxel_traverse(p["u"], p["end"], p["R"], p["i0"], p["j0"], p["k0"], p["ni"],
                                p["nj"], p["nk"], p["pitch"], p["bitmap"], p["counters"],
                                p["shortcut"], None)
    return rc, lib.anr_last_error().decode()


def _count(lib, **over):
    p = dict(bitmap=FAKE, ni=40, nj=10, nk=10, pitch=64, counts=FAKE)
    assert set(over) <= set(p)
    p.update(over)
    rc = lib.anr_voxel_count(p["bitmap"], p["ni"], p["nj"], p["nk"], p["pitch"], p["counts"], None)
    return rc, lib.anr_last_error().decode()


def _compact(lib, **over):
    p = dict(bitmap=FAKE, i0=-5, j0=-5, k0=-5, ni=40, nj=10, nk=10, pitch=64, offsets=FAKE,
             n_out=7, voxels=FAKE)
    assert set(over) <= set(p)
    p.update(over)
    rc = lib.anr_voxel_compact(p["bitmap"], p["i0"], p["j0"], p["k0"], p["ni"], p["nj"], p["nk"],
                               p["pitch"], p["offsets"], p["n_out"], p["voxels"], None)
    return rc, lib.anr_last_error().decode()


ENTRIES = {"anr_voxel_traverse": _traverse, "anr_voxel_count": _count,
           "anr_voxel_compact": _compact}
I32 = (1 << 31) - 1


@pytest.mark.parametrize("name", list(ENTRIES))
@pytest.mark.parametrize("over,word", [
    (dict(ni=0), "extents"), (dict(nj=-1), "extents"), (dict(nk=0), "extents"),
    (dict(pitch=40), "row_pitch"),     # not a multiple of 32
    (dict(pitch=32), "row_pitch"),     # shorter than a row of 40
    (dict(pitch=0), "row_pitch"), (dict(pitch=-64), "row_pitch"),
    (dict(pitch=1 << 32), "row_pitch"),
    # 2^31 * 2^15 * 2^15 = 2^61 bits, then products that leave int64
    (dict(ni=I32, pitch=1 << 31, nj=1 << 15, nk=1 << 15), "bit count"),
    (dict(ni=I32, pitch=1 << 31, nj=I32, nk=I32), "bit count"),
    (dict(nj=1 << 23, nk=1 << 17), "bit count"),  # 64 * 2^40 = 2^46 bits: the first refused
])
def test_bad_box(name, over, word):
    lib = _L()[1]
    if name != "anr_voxel_count":
        over = dict(over, i0=0, j0=0, k0=0)
    rc, msg = ENTRIES[name](lib, **over)
    assert rc == INVALID and msg.startswith(name + ":") and word in msg, (rc, msg)


@pytest.mark.parametrize("name", ["anr_voxel_traverse", "anr_voxel_compact"])
def test_box_corner_must_fit_int32(name):
    lib = _L()[1]
    for over in (dict(i0=I32 - 10), dict(j0=I32 - 5), dict(k0=I32)):
        rc, msg = ENTRIES[name](lib, **over)
        assert rc == INVALID and "overflows int32" in msg, (over, msg)
    # the most negative origin is fine: answered by the next check
    rc, msg = ENTRIES[name](lib, i0=-(1 << 31), bitmap=None)
    assert rc == INVALID and "null pointer" in msg


def test_largest_accepted_box_is_answered_by_the_next_check():
    lib = _L()[1]
    rc, msg = _count(lib, nj=1 << 23, nk=(1 << 17) - 1, counts=None)
    assert rc == INVALID and "null pointer" in msg


@pytest.mark.parametrize("name,field", [
    *[("anr_voxel_traverse", f) for f in ("u", "end", "bitmap", "counters")],
    *[("anr_voxel_count", f) for f in ("bitmap", "counts")],
    *[("anr_voxel_compact", f) for f in ("bitmap", "offsets", "voxels")],
])
def test_null_pointer(name, field):
    rc, msg = ENTRIES[name](_L()[1], **{field: None})
    assert rc == INVALID and msg.startswith(name + ": null pointer"), msg


def test_bad_counts_and_empty_calls():
    lib = _L()[1]
    for R in (-1, 1 << 31):
        rc, msg = _traverse(lib, R=R)
        assert rc == INVALID and "bad R" in msg
    rc, msg = _traverse(lib, shortcut=2)
    assert rc == INVALID and "shortcut" in msg
    # R = 0: ANR_OK without a launch, no pointer looked at; the box is still checked
    assert _traverse(lib, R=0, u=None, end=None, bitmap=None, counters=None)[0] == OK
    assert _traverse(lib, R=0, pitch=40)[0] == INVALID
    for n in (-1, 1 << 60):
        rc, msg = _compact(lib, n_out=n)
        assert rc == INVALID and "bad n_out" in msg
    assert _compact(lib, n_out=0, bitmap=None, offsets=None, voxels=None)[0] == OK
    nb = lib.anr_voxel_n_blocks
    assert [nb(n) for n in (-3, 0, 1, 1024, 1025, 1 << 30)] == [0, 0, 1, 1, 2, 1 << 20]


def test_binding_declares_the_entries():
    L, lib = _L()
    for name in ("anr_voxel_traverse", "anr_voxel_count", "anr_voxel_compact",
                 "anr_voxel_n_blocks"):
        assert name in L.symbols() and hasattr(lib, name)
    assert lib.anr_abi_version() == 5


def test_wrapper_refuses_cpu_tensors_and_big_boxes():
    from atmonr_amd import _lib
    from atmonr_amd.graphics_utils import VoxelBitmap, voxel_traversal

    u = torch.zeros(4, 3)
    with pytest.raises(_lib.ANRError, match="GPU tensors"):
        voxel_traversal(u, u + 1)
    # the limit is checked before anything is allocated
    with pytest.raises(ValueError, match=r"100000 x 100000 x 100000.*max_bitmap_bytes"):
        VoxelBitmap((0, 0, 0), (99999, 99999, 99999), "cpu")
    with pytest.raises(ValueError, match="empty"):
        VoxelBitmap((0, 0, 0), (5, -1, 5), "cpu")
    bm = VoxelBitmap((-3, 0, 0), (30, 1, 2), "cpu")
    assert bm.ext == (34, 2, 3) and bm.row_pitch == 64 and bm.n_words == 12
    lo, hi = VoxelBitmap.bounds(torch.tensor([[0.5, -0.5, 2.0], [math.nan, 9.0, 9.0]]),
                                torch.tensor([[-1.5, 3.5, 2.5], [0.0, 0.0, 0.0]]))
    assert (lo, hi) == ([-2, -1, 2], [0, 3, 2])


# ------------------------------------------------------------------ factory and dump
class _Scene:
    """As much of a dataset as the grid dataset's constructor reads."""

    device = torch.device("cpu")
    config = {"ray_origin_height": 20000.0}
    img_shp = (2, 2)
    lat = torch.tensor([[30.0], [30.0], [30.1], [30.1]])
    lon = torch.tensor([[-60.0], [-59.9], [-60.0], [-59.9]])


def test_get_extract_dataset(monkeypatch):
    from atmonr_amd import extract

    for mode in ("l1c", "voxelgrid"):
        ds = extract.get_extract_dataset(mode, _Scene(), alt_step=5000.0)
        assert type(ds) is extract.GridExtractDataset and len(ds) == 4 * 5
    made = {}

    def init(self, dataset, **kw):
        made.update(kw, dataset=dataset)

    monkeypatch.setattr(extract.GlobalGridExtractDataset, "__init__", init)
    scene = _Scene()
    ds = extract.get_extract_dataset("globalgrid", scene, scale=SCALE, grid_res=RES, vstretch=12)
    assert type(ds) is extract.GlobalGridExtractDataset
    assert made == dict(dataset=scene, scale=SCALE, grid_res=RES, vstretch=12)
    with pytest.raises(NotImplementedError, match="earthcare"):
        extract.get_extract_dataset("earthcare", scene)
    with pytest.raises(ValueError, match="coord_mode"):
        extract.get_extract_dataset("nonsense", scene)


def test_dump_writes_two_files_then_refuses(tmp_path):
    from atmonr_amd.extract import GlobalGridExtractDataset

    ds = GlobalGridExtractDataset.__new__(GlobalGridExtractDataset)
    ds.voxels = torch.tensor([[1, 2, 3], [-4, 5, 6]], dtype=torch.int32)
    sigma = torch.tensor([[0.5], [0.25]])
    ds.dump(tmp_path / "volume.vdb", sigma)
    assert sorted(p.name for p in tmp_path.iterdir()) == ["sigma.npy", "voxels.npy"]
    assert np.array_equal(np.load(tmp_path / "voxels.npy"), ds.voxels.numpy())
    assert np.load(tmp_path / "voxels.npy").dtype == np.int32
    assert np.array_equal(np.load(tmp_path / "sigma.npy"), sigma.numpy())
    with pytest.raises(FileExistsError):
        ds.dump(tmp_path / "volume.vdb", sigma)
    (tmp_path / "voxels.npy").unlink()
    with pytest.raises(FileExistsError):  # sigma.npy alone is enough
        ds.dump(tmp_path / "volume.vdb", sigma)
    assert not (tmp_path / "voxels.npy").exists()
