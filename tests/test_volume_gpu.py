"""anr_volume_render on the GPU against the f64 numpy yardstick (tests/volume_checks.py).

Tolerance of the oracle comparisons: per channel, on the pixels the yardstick does not exclude
(a decision within 1e-4 of its threshold; their share is capped in tests/test_volume_cpu.py),
the largest absolute difference to the f64 yardstick must be <= max(4 e_arm, 2^-20
max|yardstick|), e_arm being the same distance of the yardstick's own float32 arm. The factor
4 covers another evaluation order, an FMA-contracted interpolation and a device exp; it is the
convention of the field-backward oracle tests. Each case prints e_gpu and e_arm.
"""

import numpy as np
import pytest
import torch

from tests import volume_checks as vc

pytestmark = pytest.mark.gpu


def _settings(P: vc.Params):
    from atmonr_amd.video import VolumeRenderSettings

    return VolumeRenderSettings(**{k: getattr(P, k) for k in P.__dataclass_fields__})


def _render(dev, den, cams, H, W, P, **kw):
    from atmonr_amd.video import render_volume

    out = render_volume(torch.from_numpy(np.ascontiguousarray(den)).to(dev),
                        torch.from_numpy(np.ascontiguousarray(cams)).to(dev), W, H,
                        _settings(P), **kw)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("name", vc.CASES)
def test_against_the_f64_oracle(dev, name):
    """cutoff0: no density or transmittance branch exists, only step counts exclude pixels.
    down_odd: the down camera at an odd size, two direction components exactly 0 in the centre
    column. cutoff: absorb 0.5, scatter 2.0, cutoff 0.01, so that termination happens.
    channels: every coefficient different per channel, the light off-axis and not white."""
    den, cams, H, W, P = vc.case(name)
    got = _render(dev, den, cams, H, W, P).cpu().numpy()
    assert got.shape == (cams.shape[0], H, W, 4) and np.isfinite(got).all()
    e_gpu, e_arm, bound = vc.errors(name, got)
    print(f"{name}: e_gpu {e_gpu.tolist()} e_arm {e_arm.tolist()} bound {bound.tolist()} "
          f"compared {int(vc.compared_pixels(name).sum())} of {got[..., 0].size} pixels")
    assert np.all(e_gpu <= bound), (name, e_gpu, bound)
    # a miss is exactly zero, and the yardstick's misses are the kernel's
    miss = vc.reference(name)[0]["flags"][..., 3]
    assert np.all(got[miss] == 0.0)
    assert np.all(got[~miss & vc.compared_pixels(name)][:, 3] >= 0.0)


def test_analytic_slab(dev):
    """A constant cube, scatter = 0, one pixel along -z: A = 1 - exp(-absorb c step n) with n
    counted by hand (volume_checks.slab_case), L = 0. Seven f32 factors, each within an ulp or
    two: 2e-6 is ample and far below any miscounted sample (one sample changes A by 0.05)."""
    den, cam, P, alpha = vc.slab_case()
    got = _render(dev, den, cam, 1, 1, P).cpu().numpy()
    assert got.shape == (1, 1, 1, 4)
    assert np.all(got[0, 0, 0, :3] == 0.0)
    assert abs(float(got[0, 0, 0, 3]) - alpha) <= 2e-6, (got[0, 0, 0, 3], alpha)


def test_frames_are_independent(dev):
    """Three cameras in one launch equal three single-camera launches bit for bit, and so does
    a render_volume call forced to cut the frames into chunks."""
    den, cams, H, W, P = vc.case("cutoff")
    whole = _render(dev, den, cams, H, W, P)
    for f in range(cams.shape[0]):
        one = _render(dev, den, cams[f:f + 1], H, W, P)
        assert torch.equal(one[0], whole[f]), f
    # a budget of one frame, and one below a frame (still one frame per launch)
    for budget in (H * W * 16, 1):
        assert torch.equal(_render(dev, den, cams, H, W, P, max_bytes=budget), whole)
    two = _render(dev, den, cams, H, W, P, max_bytes=2 * H * W * 16)
    assert torch.equal(two, whole)


@pytest.mark.parametrize("corner", ["far", "origin"])
def test_unpadded_cube_edge(dev, corner):
    """A cube whose only nonzero voxel is the corner (nx-1, ny-1, nz-1), or (0, 0, 0): the edge
    handling must neither drop it nor wrap it into the neighbouring row of the array."""
    den = np.zeros(vc.SHAPE, np.float32)
    idx = tuple(n - 1 for n in vc.SHAPE) if corner == "far" else (0, 0, 0)
    den[idx] = 0.3
    P = vc.Params(absorb=(0.5,) * 3, scatter=(2.0,) * 3, cutoff=0.0, shadow_step=1.0)
    cams = vc.make_cameras()
    got = _render(dev, den, cams, vc.IMAGE_H, vc.IMAGE_W, P).cpu().numpy()
    want = vc.render(den, cams, vc.IMAGE_H, vc.IMAGE_W, P)
    arm = vc.render(den, cams, vc.IMAGE_H, vc.IMAGE_W, P, np.float32)
    keep = want["margin"] >= vc.MARGIN
    assert keep.mean() > 0.98
    e_gpu = np.abs(got - want["rgba"])[keep].max(axis=0)
    e_arm = np.abs(arm["rgba"] - want["rgba"])[keep].max(axis=0)
    bound = np.maximum(4 * e_arm, 2.0 ** -20 * np.abs(want["rgba"])[keep].max(axis=0))
    print(f"{corner}: e_gpu {e_gpu.tolist()} e_arm {e_arm.tolist()}")
    assert want["rgba"][..., 3].max() > 0.05  # the voxel is seen
    assert np.all(e_gpu <= bound), (e_gpu, bound)
    # seen where the yardstick sees it and nowhere else: a wrapped voxel would light pixels
    # whose rays pass the opposite face
    lit_want, lit_got = want["rgba"][..., 3] > 1e-4, got[..., 3] > 1e-4
    assert np.array_equal(lit_want[keep], lit_got[keep])


def test_make_video_writes_the_orbit_frames(dev, tmp_path):
    from atmonr_amd.video import make_video, orbit_cameras, read_ppm, render_volume, write_ppm

    rng = np.random.default_rng(2)
    ext = rng.uniform(0.0, 0.3, (6, 7, 5, 4)).astype(np.float32)  # (H, W, A, bands)
    ext[0, 0, 0, 2] = np.nan
    np.savez(tmp_path / "extract.npz", extinction=ext)
    res = make_video(tmp_path / "extract.npz", tmp_path / "frames", None, width=32, height=24,
                     duration=1.0, frame_rate=4, device=dev)
    assert res["shape"] == (7, 5, 6) and res["video"] is None and "frames stay" in res["ffmpeg"]
    names = sorted(p.name for p in (tmp_path / "frames").iterdir())
    assert names == ["000000.ppm", "000001.ppm", "000002.ppm", "000003.ppm"]
    head = b"P6\n32 24\n255\n"
    for p in res["frames"]:
        raw = open(p, "rb").read()
        assert raw.startswith(head) and len(raw) == len(head) + 32 * 24 * 3
    from atmonr_amd.video import volume_from_extract

    cube = torch.from_numpy(volume_from_extract(ext)).to(dev)
    cams = orbit_cameras(cube.shape, 1.0, 4, 32, 24, device=dev)
    first = render_volume(cube, cams, 32, 24)[0]
    write_ppm(tmp_path / "first.ppm", first)
    assert open(tmp_path / "first.ppm", "rb").read() == open(res["frames"][0], "rb").read()
    assert read_ppm(res["frames"][0]).max() > 20  # the cloud is lit, not a black frame
