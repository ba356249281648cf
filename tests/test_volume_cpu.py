"""The volume ray marcher without a GPU: anr_volume_render is declared, exported, bound and
refuses what it cannot take before any launch; the numpy yardstick (tests/volume_checks.py)
gives the answers known by hand; the host layer (atmonr_amd.video) restates the script's
formulas; and the inputs of tests/test_volume_gpu.py satisfy the conditions those tests rely
on. No kernel runs."""

import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

from tests import volume_checks as vc
from tests.conftest import ROOT

FAKE = 0x10000  # a non-null, 16-byte aligned address that is never dereferenced


def _params(**kw):
    from atmonr_amd.video import VolumeRenderSettings

    return VolumeRenderSettings(**kw).params()


def _call(dims=(7, 5, 6), F=3, H=16, W=24, density=FAKE, cams=FAKE, out=FAKE, params="default",
          **kw):
    from atmonr_amd import _lib

    lib = _lib.load()
    p = _params(**kw) if params == "default" else params
    rc = lib.anr_volume_render(density, *dims, cams, F, H, W,
                               ctypes.byref(p) if p is not None else None, out, None)
    return rc, lib.anr_last_error().decode()


def test_symbol_is_declared_exported_and_bound():
    from atmonr_amd import _lib

    src = open(os.path.join(ROOT, "include", "anr.h")).read()
    assert "vdb_render: unpinned" in src
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert re.search(r"\banr_volume_render\s*\(", code)
    assert "anr_volume_render" in _lib.symbols()
    assert hasattr(_lib.load(), "anr_volume_render")
    assert _lib.load().anr_abi_version() == 5
    assert re.search(r"#define ANR_ABI_VERSION 5\b", code)
    # the POD structs are what the header declares: 12 and 16 floats
    assert ctypes.sizeof(_lib.Camera) == 48 and ctypes.sizeof(_lib.VolumeParams) == 64
    assert re.search(r"float eye\[3\], forward\[3\], right\[3\], up\[3\];\s*}\s*anr_camera;", code)


@pytest.mark.parametrize("F,H,W", [(0, 16, 24), (3, 0, 24), (3, 16, 0)])
def test_no_pixels_is_a_no_op_success(F, H, W):
    rc, msg = _call(F=F, H=H, W=W, density=None, cams=None, out=None)
    assert rc == 0, msg


REFUSALS = {
    "null_density": (dict(density=None), "null pointer"),
    "null_cameras": (dict(cams=None), "null pointer"),
    "null_output": (dict(out=None), "null pointer"),
    "null_params": (dict(params=None), "null pointer"),
    "zero_extent": (dict(dims=(7, 0, 6)), "extents"),
    "negative_extent": (dict(dims=(-1, 5, 6)), "extents"),
    "negative_image": (dict(H=-1), "image size"),
    "zero_primary_step": (dict(primary_step=0.0), "steps must be positive"),
    "negative_shadow_step": (dict(shadow_step=-3.0), "steps must be positive"),
    "nan_step": (dict(primary_step=float("nan")), "steps must be positive"),
    "negative_absorb": (dict(absorb=(0.1, -0.1, 0.1)), "negative coefficient"),
    "negative_scatter": (dict(scatter=(0.7, 0.7, -1e-3)), "negative coefficient"),
    "negative_light_color": (dict(light_color=(-1.0, 1.0, 1.0)), "negative coefficient"),
    "negative_gain": (dict(light_gain=-0.2), "negative coefficient"),
    "negative_cutoff": (dict(cutoff=-0.01), "negative coefficient"),
    "light_not_unit": (dict(light_dir=(0.0, 1.01, 0.0)), "unit length"),
    "light_zero": (dict(light_dir=(0.0, 0.0, 0.0)), "unit length"),
    "cube_2gib": (dict(dims=(1024, 1024, 512)), "2^31 bytes"),
    "cube_overflow": (dict(dims=(1 << 40, 1 << 40, 1 << 40)), "2^31 bytes"),
}


@pytest.mark.parametrize("case", sorted(REFUSALS))
def test_refusals_carry_a_message(case):
    """Every refusal comes back before a launch (the pointers are fake) as ANR_E_INVALID with
    the entry's name and the reason in anr_last_error."""
    kw, word = REFUSALS[case]
    rc, msg = _call(**kw)
    assert rc == -1, (rc, msg)
    assert "anr_volume_render" in msg and word in msg, msg


def test_light_dir_within_a_thousandth_is_accepted_up_to_the_pointer_check():
    # |light_dir| = 1.0005 passes the unit test; the call then fails on the null output only
    rc, msg = _call(light_dir=(0.0, 1.0005, 0.0), out=None)
    assert rc == -1 and "null pointer" in msg, msg


# ------------------------------------------------------------------ the yardstick's known answers
def test_oracle_constant_slab_matches_the_hand_count():
    den, cam, P, alpha = vc.slab_case()
    for dtype, tol in ((np.float64, 1e-12), (np.float32, 1e-6)):
        out = vc.render(den, cam, 1, 1, P, dtype)
        assert out["rgba"].shape == (1, 1, 1, 4)
        assert np.all(out["rgba"][0, 0, 0, :3] == 0.0)  # scatter = 0: no light
        assert abs(out["rgba"][0, 0, 0, 3] - alpha) <= tol
        assert not out["flags"].any()  # cutoff 0: no branch fires, and the ray is no miss
        # n + 1 primary samples, each with one shadow sample: from y = 2 the light's way out of
        # the box is 3 long, one shadow step
        assert out["lookups"][0, 0, 0] == 2 * (den.shape[2] + 1)
    assert 0.3 < alpha < 0.5


def test_oracle_empty_cube_and_missing_ray_are_zero():
    cams = vc.make_cameras()
    out = vc.render(np.zeros(vc.SHAPE, np.float32), cams, 4, 6, vc.Params())
    assert np.all(out["rgba"] == 0.0)
    # a camera that looks away from the cube misses it in every pixel
    away = vc.look_at((20.0, 3.0, 3.0), (40.0, 3.0, 3.0), (0.0, 1.0, 0.0), 4, 6)[None]
    out = vc.render(vc.make_cube(11), away, 4, 6, vc.Params())
    assert np.all(out["rgba"] == 0.0) and out["flags"][..., 3].all()
    assert np.all(out["lookups"] == 0)


def test_oracle_zero_direction_component():
    """A direction component of exactly 0: the axis constrains nothing while the eye is in
    its slab, and the ray misses once it is not."""
    den = np.full((5, 5, 6), 0.2, np.float32)
    P = vc.Params(cutoff=0.0)
    inside = vc.look_at((2.0, 2.0, 9.0), (2.0, 2.0, 0.0), (0.0, 1.0, 0.0), 1, 1)[None]
    assert list(inside[0, 3:6]) == [0.0, 0.0, -1.0]
    assert vc.render(den, inside, 1, 1, P)["rgba"][0, 0, 0, 3] > 0.1
    outside = vc.look_at((5.5, 2.0, 9.0), (5.5, 2.0, 0.0), (0.0, 1.0, 0.0), 1, 1)[None]
    out = vc.render(den, outside, 1, 1, P)
    assert out["flags"][0, 0, 0, 3] and np.all(out["rgba"] == 0.0)
    # the slab's own faces belong to it: D is 0 there, and the ray is no miss
    edge = vc.look_at((5.0, 2.0, 9.0), (5.0, 2.0, 0.0), (0.0, 1.0, 0.0), 1, 1)[None]
    out = vc.render(den, edge, 1, 1, P)
    assert not out["flags"][0, 0, 0, 3] and np.all(out["rgba"] == 0.0)


def test_oracle_mirror_symmetric_cube_gives_a_mirror_symmetric_image():
    rng = np.random.default_rng(3)
    half = rng.uniform(0.0, 0.3, (3, 5, 6))
    den = np.concatenate([half, half[:1] * 0 + rng.uniform(0, 0.3, (1, 5, 6)), half[::-1]])
    den = den.astype(np.float32)  # (7, 5, 6), den[i] == den[6 - i]
    assert np.array_equal(den, den[::-1])
    cam = vc.look_at((3.0, 4.0, 15.0), (3.0, 1.0, 2.5), (0.0, 1.0, 0.0), 6, 8)[None]
    P = vc.Params(absorb=(0.5,) * 3, scatter=(2.0,) * 3, light_dir=vc._unit((0.0, 0.8, 0.6)),
                  shadow_step=1.0)
    out = vc.render(den, cam, 6, 8, P)["rgba"][0]
    assert out[..., 3].max() > 0.3
    assert np.abs(out - out[:, ::-1]).max() < 1e-12


def test_oracle_arms_agree_and_flags_have_the_documented_order():
    assert vc.FLAGS == ("density_skip", "shadow_terminate", "pixel_terminate", "miss")
    y, arm = vc.reference("down_odd")
    assert y["rgba"].shape == (1, 3, 5, 4)
    assert 0 < np.abs(arm["rgba"] - y["rgba"]).max() < 1e-5
    # the centre column and row of the odd image look along directions with exact zeros
    den, cams, H, W, P = vc.case("down_odd")
    assert list(cams[0, 3:6]) == [0.0, -1.0, 0.0]
    assert cams[0, 7] == 0.0 and cams[0, 8] == 0.0 and cams[0, 9] == 0.0 and cams[0, 10] == 0.0


# ------------------------------------------------------------------ the host layer
def test_orbit_cameras_follow_the_script():
    from atmonr_amd.video import DEFAULT_HFOV, orbit_cameras

    assert DEFAULT_HFOV == pytest.approx(2 * math.atan(41.2136 / 100.0), rel=1e-15)
    shape = (31, 9, 17)
    cams = orbit_cameras(shape, duration=2.0, frame_rate=6, width=64, height=48, device="cpu")
    assert cams.shape == (12, 12) and cams.dtype == torch.float32
    cams = cams.numpy().astype(np.float64)
    # scripts/make_video.py:155-169
    times = np.linspace(0, 2.0, 12)
    center = (shape[0] / 2, shape[1] / 2, shape[2] / 2)
    radius = 1.3 * np.linalg.norm(shape)
    t_circle = 2 * np.pi * times / 2.0
    orbit_x = np.cos(t_circle) * radius + center[0]
    orbit_y = np.sin(t_circle) * radius + center[2]
    height = 0.5 * np.linalg.norm(shape)
    assert np.allclose(cams[:, 0], orbit_x, rtol=1e-6, atol=1e-5)
    assert np.allclose(cams[:, 1], height, rtol=1e-6)
    assert np.allclose(cams[:, 2], orbit_y, rtol=1e-6, atol=1e-5)
    lookat = np.array([center[0], 0.0, center[2]])
    th = math.tan(DEFAULT_HFOV / 2)
    for c in cams:
        eye, fwd, right, up = c[0:3], c[3:6], c[6:9], c[9:12]
        want = (lookat - eye) / np.linalg.norm(lookat - eye)
        assert np.allclose(fwd, want, atol=1e-6)
        assert abs(fwd @ right) < 1e-6 and abs(fwd @ up) < 1e-6 and abs(right @ up) < 1e-6
        assert np.linalg.norm(right) == pytest.approx(th, rel=1e-6)
        assert np.linalg.norm(up) == pytest.approx(th * 48 / 64, rel=1e-6)
        assert right[1] == pytest.approx(0.0, abs=1e-7) and up[1] > 0  # world up is +y
        assert np.allclose(np.cross(fwd, up / np.linalg.norm(up)), right / th, atol=1e-6)
    # linspace includes its end point: the first and the last frame coincide
    assert np.allclose(cams[0], cams[-1], atol=1e-5)
    # the cameras agree with the yardstick's own look-at
    assert np.allclose(cams[3], vc.look_at(cams[3, 0:3], lookat, (0, 1, 0), 48, 64), atol=1e-6)


def test_volume_from_extract_axis_order(tmp_path):
    from atmonr_amd.video import volume_from_extract

    H, W, A, B = 4, 3, 5, 4
    ext = np.arange(H * W * A * B, dtype=np.float32).reshape(H, W, A, B) + 1.0
    ext[2, 1, 4, 2] = np.nan
    ext[0, 0, 0, 1] = np.nan
    cube = volume_from_extract(ext)
    assert cube.shape == (W, A, H) and cube.dtype == np.float32 and cube.flags["C_CONTIGUOUS"]
    # scripts/make_video.py:146-148 on the same array
    want = np.ascontiguousarray(np.transpose(ext[:, :, ::-1, 2], (1, 2, 0)))
    assert np.array_equal(np.nan_to_num(want, nan=0.0), cube)
    assert cube[1, 0, 2] == 0.0  # the NaN: altitude index 4 flips to y = 0
    assert cube[2, 4, 3] == ext[3, 2, 0, 2]  # (w, flipped a, h)
    # band and scale are honoured
    c1 = volume_from_extract(ext, band=1, scene_scale=2500.0)
    assert c1[0, A - 1, 0] == 0.0 and c1[2, 1, 3] == pytest.approx(ext[3, 2, 3, 1] * 2.5)
    # the .npz that GridExtractDataset.dump writes
    np.savez(tmp_path / "extract.npz", extinction=ext, sample_alt=np.arange(A))
    assert np.array_equal(volume_from_extract(tmp_path / "extract.npz"), cube)
    assert np.array_equal(volume_from_extract(torch.from_numpy(ext)), cube)
    from atmonr_amd._lib import ANRError
    with pytest.raises(ANRError, match="band"):
        volume_from_extract(ext, band=4)
    with pytest.raises(ANRError, match="bands"):
        volume_from_extract(ext[..., 0])


def test_write_ppm_round_trip(tmp_path):
    from atmonr_amd.video import read_ppm, write_ppm

    rng = np.random.default_rng(0)
    img = rng.uniform(-0.2, 1.2, (5, 7, 4))
    img[0, 0] = [0.0, 1.0, 0.5, 0.3]
    img[0, 1] = [np.nan, 2.0, -1.0, 0.0]
    write_ppm(tmp_path / "a.ppm", img)
    raw = open(tmp_path / "a.ppm", "rb").read()
    assert raw.startswith(b"P6\n7 5\n255\n") and len(raw) == len(b"P6\n7 5\n255\n") + 5 * 7 * 3
    got = read_ppm(tmp_path / "a.ppm")
    want = np.rint(np.clip(np.nan_to_num(img[..., :3]), 0, 1) * 255).astype(np.uint8)
    assert np.array_equal(got, want)
    assert list(got[0, 0]) == [0, 255, 128] and list(got[0, 1]) == [0, 255, 0]
    # 8-bit values survive a second trip unchanged; a tensor is taken as well
    write_ppm(tmp_path / "b.ppm", torch.from_numpy(got.astype(np.float32) / 255.0))
    assert np.array_equal(read_ppm(tmp_path / "b.ppm"), got)


def test_render_volume_refuses_cpu_tensors():
    from atmonr_amd._lib import ANRError
    from atmonr_amd.video import render_volume

    with pytest.raises(ANRError, match="GPU"):
        render_volume(torch.zeros(3, 3, 3), torch.zeros(1, 12), 8, 8)


def test_settings_defaults_and_cli_options():
    from atmonr_amd.video import VolumeRenderSettings

    p = VolumeRenderSettings().params()
    assert (p.primary_step, p.shadow_step) == (1.0, 3.0)
    assert p.light_gain == pytest.approx(0.2) and p.cutoff == pytest.approx(0.01)
    assert list(p.absorb) == pytest.approx([0.1] * 3) and list(p.scatter) == pytest.approx([0.7] * 3)
    assert list(p.light_dir) == [0.0, 1.0, 0.0] and list(p.light_color) == [1.0, 1.0, 1.0]
    d = vc.Params()
    s = VolumeRenderSettings()
    assert all(getattr(d, k) == getattr(s, k) for k in d.__dataclass_fields__)
    # tools/make_video.py keeps the reference script's argument names
    import importlib.util

    spec = importlib.util.spec_from_file_location("make_video_tool",
                                                  os.path.join(ROOT, "tools", "make_video.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    opts = {a.option_strings[0] for a in tool.build_parser()._actions if a.option_strings}
    for name in ("--extract-filepath", "--video-filepath", "--render-band-idx", "--res",
                 "--frame-rate", "--duration", "--absorb", "--cutoff", "--light-source-dir",
                 "--light-source-color", "--scatter"):
        assert name in opts, name
    args = tool.build_parser().parse_args(["--extract-filepath", "x.npz", "--video-filepath",
                                           "x.mp4"])
    assert args.res == "640x480" and args.frame_rate == 60 and args.duration == 10.0
    assert tuple(args.absorb) == (0.1, 0.1, 0.1) and tuple(args.scatter) == (0.7, 0.7, 0.7)
    assert args.cutoff == 0.01 and tuple(args.light_source_dir) == (0.0, 1.0, 0.0)


# ------------------------------------------------------------------ what the GPU tests rely on
@pytest.mark.parametrize("name", vc.CASES)
def test_gpu_case_inputs_satisfy_the_conditions(name):
    """For the exact seeds and shapes of tests/test_volume_gpu.py, by the f64 yardstick alone:
    at most 2 % of an image's pixels have a decision within 1e-4 of its threshold (they are
    left out of the comparison there); with a cutoff each of the three branches fires in at
    least 10 % of the pixels that hit the box; and some pixel misses the box."""
    den, cams, H, W, P = vc.case(name)
    y, arm = vc.reference(name)
    assert den.shape == vc.SHAPE and den.min() == 0.0 and 0.25 < den.max() <= 0.3
    assert np.all(den[1:3, 1:3, 3:5] == 0.0)
    excluded = y["margin"] < vc.MARGIN
    for f in range(cams.shape[0]):
        assert excluded[f].mean() <= 0.02, (name, f, excluded[f].mean())
    miss = y["flags"][..., 3]
    if name != "down_odd":
        assert (H, W, cams.shape[0]) == (16, 24, 3)
        assert miss.any()
        assert not miss[1].any() and not miss[2].all()  # the inside camera sees the cube everywhere
    if P.cutoff > 0:
        for b, flag in enumerate(vc.FLAGS[:3]):
            share = y["flags"][..., b][~miss].mean()
            assert share >= 0.10, (name, flag, share)
    else:
        assert not y["flags"][..., :3].any()
    # on the compared pixels the f32 arm takes the f64 yardstick's branches
    keep = vc.compared_pixels(name)
    assert np.array_equal(arm["flags"][keep], y["flags"][keep])
    e_got, e_arm, bound = vc.errors(name, arm["rgba"])
    assert np.all(e_got == e_arm) and np.all(e_arm > 0) and np.all(bound < 1e-5)
