"""The include_height coordinate: anr_append_heights and the fused sampler's mode 2 against
the reference's own ``append_heights`` (tests/golden/append_heights.npz, written by
tools/gen_append_heights_golden.py from the reference on the CPU).

Bound on the height: |h - h_ref| <= max(one f32 ulp of h_ref, 1e-9). Both sides evaluate
the Bowring altitude in f64, where it carries a few ulps of 6.4e6 m of cancellation error;
divided by ray_origin_height = 2e4 m that is ~1e-13, so only a flip at an f32 rounding
boundary can move the result, and by one ulp. Columns 0-2 are copies: bit-equal."""

import numpy as np
import pytest
import torch

from tests.conftest import golden

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fix():
    g = golden("append_heights.npz")
    return {k: g[k] for k in g.files}


def _check_heights(h, h_ref):
    h = np.asarray(h, dtype=np.float64)
    ref32 = np.asarray(h_ref, dtype=np.float32)
    bound = np.maximum(np.spacing(np.abs(ref32)).astype(np.float64), 1e-9)
    err = np.abs(h - ref32.astype(np.float64))
    print(f"height: max err {err.max():.3e}, rows off by an ulp {(err > 0).sum()} of {err.size}")
    assert np.all(err <= bound), f"max err {err.max():.3e} at {err.argmax()}"


def _args(fix):
    return (float(fix["ray_origin_height"]), float(fix["scale"]),
            torch.from_numpy(fix["offset"]))


def test_append_heights_f32_vs_reference(dev, fix):
    from atmonr_amd.samplers import append_heights

    pts = torch.from_numpy(fix["pts_f32"]).to(dev).view(64, 64, 3)
    out = append_heights(pts, *_args(fix))
    assert out.shape == (64, 64, 4) and out.dtype == torch.float32
    out = out.view(-1, 4).cpu().numpy()
    assert np.array_equal(out[:, :3].view(np.uint32), fix["out_f32"][:, :3].view(np.uint32))
    _check_heights(out[:, 3], fix["out_f32"][:, 3])
    assert fix["out_f32"][:, 3].min() < -0.1 and fix["out_f32"][:, 3].max() > 1.5  # oddity 2


def test_append_heights_f64_vs_reference(dev, fix):
    from atmonr_amd.samplers import append_heights

    pts = torch.from_numpy(fix["pts_f64"]).to(dev).view(1, 4096, 3)
    out = append_heights(pts, *_args(fix))
    assert out.shape == (1, 4096, 4) and out.dtype == torch.float64
    out = out[0].cpu().numpy()
    assert np.array_equal(out[:, :3].view(np.uint64), fix["out_f64"][:, :3].view(np.uint64))
    assert np.array_equal(out[:, 3], out[:, 3].astype(np.float32).astype(np.float64))
    _check_heights(out[:, 3], fix["out_f64"][:, 3])


@pytest.mark.parametrize("f64", [False, True])
def test_remapped_rows_follow_the_reference_order(dev, fix, f64):
    """anr_append_heights with the Instant-NGP remap, as InstantNGPPipeline.extract uses it:
    (p + 1) / 2, the height of the remapped point, column 2 alone divided by
    alt_compress_factor -- in f64 for f64 points, rounded to f32 once."""
    from atmonr_amd import _lib
    from atmonr_amd.samplers import append_heights, points_with_heights

    roh, scale, offset = _args(fix)
    dt = torch.float64 if f64 else torch.float32
    raw = (torch.rand(4096, 3, generator=torch.Generator().manual_seed(2), dtype=dt) * 2
           - 1).to(dev)
    prep = _lib.height_params(scale, offset, roh, ngp_remap=True, alt_compress=8.0)
    out = points_with_heights(raw, prep)
    assert out.shape == (4096, 4) and out.dtype == torch.float32
    # the same steps one by one (the plain append_heights is pinned to the reference above)
    want = append_heights(((raw + 1) / 2)[None], roh, scale, offset)[0]
    assert want.dtype == dt
    want[:, 2] = want[:, 2] / 8
    assert torch.equal(out.view(torch.int32), want.float().view(torch.int32))


def _rays(dev, B, seed=0):
    gen = torch.Generator().manual_seed(seed)
    d = torch.randn(B, 3, generator=gen)
    return {"origin": (torch.rand(B, 3, generator=gen) * 2 - 1).to(dev),
            "dir": (d / d.norm(dim=1, keepdim=True)).to(dev),
            "len": (torch.rand(B, generator=gen) + 0.5).to(dev)}


@pytest.mark.parametrize("with_u", [True, False])
@pytest.mark.parametrize("B,N", [(37, 64), (3, 1024)])
def test_fused_sampler_rows_equal_the_separate_steps(dev, fix, with_u, B, N):
    """Mode 2 of the sampler kernel against sampler, remap, anr_append_heights and
    compression as separate steps: bit for bit, with draws given and with bin midpoints."""
    from atmonr_amd import _lib
    from atmonr_amd.samplers import append_heights, sample_and_preprocess, sample_uniform_bins

    roh, scale, offset = _args(fix)
    rays = _rays(dev, B)
    u = torch.rand(B, N, generator=torch.Generator().manual_seed(1)).to(dev) if with_u else None
    prep = _lib.height_params(scale, offset, roh, ngp_remap=True, alt_compress=8.0)
    pts_f, z_f, coords = sample_and_preprocess(rays, N, prep, random=False, u=u, want_pts=True)
    assert coords.shape == (B, N, 4)
    pts, z = sample_uniform_bins(rays, N, random=False, u=u)
    assert torch.equal(z_f, z) and torch.equal(pts_f, pts)
    want = append_heights((pts + 1) / 2, roh, scale, offset)
    want[..., 2] = want[..., 2] / 8
    assert torch.equal(coords.view(torch.int32), want.view(torch.int32))
    # mode 0 through the same kernel: the raw points, remapped and compressed
    prep0 = _lib.height_params(scale, offset, roh, ngp_remap=True, alt_compress=8.0,
                               append_height=False)
    _, z0, c0 = sample_and_preprocess(rays, N, prep0, random=False, u=u)
    assert c0.shape == (B, N, 3) and torch.equal(z0, z)
    assert torch.equal(c0, want[..., :3])


def test_height_entry_points_validate_their_arguments(dev, fix):
    from atmonr_amd import _lib
    from atmonr_amd.samplers import points_with_heights, preprocess_points

    roh, scale, offset = _args(fix)
    pts = torch.rand(5, 3, device=dev)
    with pytest.raises(_lib.ANRError, match="mode"):
        points_with_heights(pts, _lib.height_params(scale, offset, roh, append_height=False))
    with pytest.raises(_lib.ANRError, match="mode"):  # 3-wide entry points refuse mode 2
        preprocess_points(pts, _lib.height_params(scale, offset, roh))
    assert points_with_heights(pts[:0], _lib.height_params(scale, offset, roh)).shape == (0, 4)
