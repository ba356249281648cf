"""The sparse volume without a GPU: its entries are declared, exported, bound and refuse what
they cannot take before any launch; the orbit about the local vertical has the geometry the
host layer documents; the command-line tool parses its options; and the inputs of
tests/test_sparse_volume_gpu.py satisfy the conditions those tests rely on."""

import ctypes
import importlib.util
import os
import re

import numpy as np
import pytest
import torch

from tests import sparse_volume_checks as sc
from tests import volume_checks as vc
from tests.conftest import ROOT

FAKE = 0x10000  # a non-null, 16-byte aligned address that is never dereferenced
ENTRIES = ("anr_sparse_volume_coarse_words", "anr_sparse_volume_mark",
           "anr_sparse_volume_popcount", "anr_sparse_volume_place", "anr_sparse_volume_sample",
           "anr_sparse_volume_render")


def test_entries_are_declared_exported_and_bound():
    from atmonr_amd import _lib

    src = open(os.path.join(ROOT, "include", "anr.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name in ENTRIES:
        assert re.search(r"\b%s\s*\(" % name, code), name
        assert name in _lib.symbols() and hasattr(_lib.load(), name)
        assert name in src.split("#define ANR_ABI_VERSION")[0]  # listed under "added to ABI 5"
    assert _lib.load().anr_abi_version() == 5
    assert ctypes.sizeof(_lib.SparseVolumeDesc) == 56
    assert re.search(r"int64_t n_values;\s*}\s*anr_sparse_volume;", code)


def _desc(ni=70, nj=9, nk=11, row_pitch=96, n_values=100, cells=FAKE, values=FAKE, coarse=FAKE):
    from atmonr_amd import _lib

    d = _lib.SparseVolumeDesc()
    d.cells, d.values, d.coarse = cells, values, coarse
    d.ni, d.nj, d.nk, d.reserved, d.row_pitch, d.n_values = ni, nj, nk, 0, row_pitch, n_values
    return d


def _render(desc="default", skip=1, F=3, H=16, W=24, cams=FAKE, out=FAKE, params="default", **kw):
    from atmonr_amd import _lib
    from atmonr_amd.video import VolumeRenderSettings

    lib = _lib.load()
    d = _desc() if desc == "default" else desc
    p = VolumeRenderSettings(**kw).params() if params == "default" else params
    rc = lib.anr_sparse_volume_render(ctypes.byref(d) if d is not None else None, skip, cams, F,
                                      H, W, ctypes.byref(p) if p is not None else None, out,
                                      None, None)
    return rc, lib.anr_last_error().decode()


def _sample(desc="default", skip=1, pos=FAKE, P=10, out=FAKE):
    from atmonr_amd import _lib

    lib = _lib.load()
    d = _desc() if desc == "default" else desc
    rc = lib.anr_sparse_volume_sample(ctypes.byref(d) if d is not None else None, skip, pos, P,
                                      out, None)
    return rc, lib.anr_last_error().decode()


VOLUME_REFUSALS = {
    "null_volume": (dict(desc=None), "null pointer"),
    "null_cells": (dict(desc=_desc(cells=None)), "null pointer"),
    "null_values": (dict(desc=_desc(values=None)), "null pointer"),
    "null_coarse_with_skip": (dict(desc=_desc(coarse=None)), "null pointer"),
    "zero_extent": (dict(desc=_desc(nj=0)), "extents"),
    "negative_extent": (dict(desc=_desc(ni=-1)), "extents"),
    "pitch_below_ni": (dict(desc=_desc(row_pitch=64)), "row_pitch"),
    "pitch_not_32": (dict(desc=_desc(row_pitch=100)), "row_pitch"),
    "words_2_31": (dict(desc=_desc(ni=1 << 12, nj=1 << 14, nk=1 << 12, row_pitch=1 << 12)),
                   "2^31 bitmap words"),
    "no_values": (dict(desc=_desc(n_values=0)), "n_values"),
    "values_2_31": (dict(desc=_desc(n_values=1 << 31)), "n_values"),
    "bad_skip": (dict(skip=2), "skip"),
}
RENDER_REFUSALS = {
    "null_cameras": (dict(cams=None), "null pointer"),
    "null_output": (dict(out=None), "null pointer"),
    "null_params": (dict(params=None), "null pointer"),
    "negative_image": (dict(H=-1), "image size"),
    "zero_primary_step": (dict(primary_step=0.0), "steps must be positive"),
    "nan_step": (dict(shadow_step=float("nan")), "steps must be positive"),
    "negative_absorb": (dict(absorb=(0.1, -0.1, 0.1)), "negative coefficient"),
    "negative_cutoff": (dict(cutoff=-0.01), "negative coefficient"),
    "light_not_unit": (dict(light_dir=(0.0, 1.01, 0.0)), "unit length"),
}


@pytest.mark.parametrize("case", sorted(VOLUME_REFUSALS))
def test_volume_refusals_carry_a_message(case):
    kw, word = VOLUME_REFUSALS[case]
    rc, msg = _render(**kw)
    assert rc == -1 and "anr_sparse_volume_render" in msg and word in msg, (rc, msg)
    rc, msg = _sample(**kw)
    assert rc == -1 and "anr_sparse_volume_sample" in msg and word in msg, (rc, msg)


@pytest.mark.parametrize("case", sorted(RENDER_REFUSALS))
def test_render_refusals_are_the_dense_entry_s(case):
    kw, word = RENDER_REFUSALS[case]
    rc, msg = _render(**kw)
    assert rc == -1 and "anr_sparse_volume_render" in msg and word in msg, (rc, msg)


def test_no_work_is_a_no_op_success_and_skip_0_needs_no_coarse():
    for kw in (dict(F=0), dict(H=0), dict(W=0)):
        rc, msg = _render(cams=None, out=None, **kw)
        assert rc == 0, msg
    assert _sample(pos=None, out=None, P=0)[0] == 0
    assert _sample(P=-1)[0] == -1
    # without the brick level a null coarse passes; the call then fails on the null output only
    rc, msg = _render(desc=_desc(coarse=None), skip=0, out=None)
    assert rc == -1 and "null pointer" in msg
    # a box whose dense cube anr_volume_render refuses (2.69 GB) is accepted up to that point
    rc, msg = _render(desc=_desc(973, 873, 791, 992, 78_300_000), out=None)
    assert rc == -1 and "null pointer" in msg, msg


def test_build_entries_refuse_before_a_launch():
    from atmonr_amd import _lib

    lib = _lib.load()
    box = (-37, 4090, -5, 70, 9, 11, 96)

    def msg():
        return lib.anr_last_error().decode()

    assert lib.anr_sparse_volume_mark(FAKE, 0, *box, FAKE, FAKE, None) == -1 and "no voxels" in msg()
    assert lib.anr_sparse_volume_mark(FAKE, 1 << 31, *box, FAKE, FAKE, None) == -1 and "2^31" in msg()
    assert lib.anr_sparse_volume_mark(None, 5, *box, FAKE, FAKE, None) == -1 and "null" in msg()
    assert lib.anr_sparse_volume_mark(FAKE, 5, 0, 0, 0, 70, 9, 11, 64, FAKE, FAKE, None) == -1
    assert "row_pitch" in msg()
    assert lib.anr_sparse_volume_mark(FAKE, 5, (1 << 31) - 10, 0, 0, 70, 9, 11, 96, FAKE, FAKE,
                                      None) == -1 and "overflows int32" in msg()
    assert lib.anr_sparse_volume_popcount(FAKE, 0, FAKE, None) == -1 and "n_words" in msg()
    assert lib.anr_sparse_volume_popcount(FAKE, 1 << 31, FAKE, None) == -1
    assert lib.anr_sparse_volume_popcount(None, 5, FAKE, None) == -1 and "null" in msg()
    assert lib.anr_sparse_volume_place(FAKE, FAKE, 0, 1.0, *box, FAKE, 5, FAKE, None) == -1
    assert lib.anr_sparse_volume_place(FAKE, FAKE, 5, float("nan"), *box, FAKE, 5, FAKE,
                                       None) == -1 and "density_scale" in msg()
    assert lib.anr_sparse_volume_place(FAKE, None, 5, 1.0, *box, FAKE, 5, FAKE, None) == -1
    # bricks: (n >> 3) + 1 per axis, 32 to a word
    assert lib.anr_sparse_volume_coarse_words(70, 9, 11) == (9 * 2 * 2 + 31) // 32
    assert lib.anr_sparse_volume_coarse_words(973, 873, 791) == (122 * 110 * 99 + 31) // 32
    assert lib.anr_sparse_volume_coarse_words(0, 9, 11) == 0


def test_host_layer_refuses_cpu_tensors_and_bad_shapes():
    from atmonr_amd._lib import ANRError
    from atmonr_amd.sparse_volume import (SparseVolume, make_global_video, render_sparse_volume,
                                          voxel_edge)

    v = torch.zeros((4, 3), dtype=torch.int32)
    with pytest.raises(ANRError, match="GPU"):
        SparseVolume.from_voxels(v, torch.zeros(4))
    with pytest.raises(ANRError, match="SparseVolume"):
        render_sparse_volume(torch.zeros(3, 3, 3), torch.zeros(1, 12), 8, 8)
    with pytest.raises(ANRError, match="band"):
        SparseVolume.from_files(np.zeros((4, 3), np.int32), np.zeros((4, 2), np.float32), band=2)
    with pytest.raises(ANRError, match="bands"):
        SparseVolume.from_files(np.zeros((4, 3), np.int32), np.zeros(4, np.float32))
    with pytest.raises(ANRError, match="sigma"):
        make_global_video(np.zeros((4, 3), np.int32), "unused")
    from atmonr_amd.geospatial.spherical import EARTH_RADIUS

    assert voxel_edge(0.025) == 0.025 / (100 / EARTH_RADIUS)
    assert voxel_edge(0.05, 2.0) == 0.025
    with pytest.raises(ANRError, match="positive"):
        voxel_edge(0.0)


class _Box:
    def __init__(self, lo, ext):
        self.lo, self.ext = lo, ext


@pytest.mark.parametrize("lo,ext", [(sc.SHELL_LO, sc.SHELL_EXT), ((-4100, -300, 2500), (973, 873, 791)),
                                    ((10, 20, -7000), (5, 6, 7))])
def test_global_orbit_cameras_geometry(lo, ext):
    from atmonr_amd.sparse_volume import global_orbit_cameras, global_settings, global_vertical
    from atmonr_amd.video import DEFAULT_HFOV

    box = _Box(lo, ext)
    up = global_vertical(box)
    c = np.asarray(lo, float) + np.asarray(ext, float) / 2
    assert np.allclose(up, c / np.linalg.norm(c), atol=1e-15) and abs(np.linalg.norm(up) - 1) < 1e-15
    assert global_settings(box).light_dir == tuple(up.tolist())
    assert global_settings(box, cutoff=0.0).cutoff == 0.0 and global_settings(box).cutoff == 0.01
    W, H = 64, 48
    cams = global_orbit_cameras(box, 2.0, 8, W, H, device="cpu")
    assert cams.shape == (16, 12) and cams.dtype == torch.float32
    cams = cams.numpy().astype(np.float64)
    assert np.array_equal(cams[0], cams[-1])  # first and last frame coincide
    assert not np.allclose(cams[0, :3], cams[8, :3])
    centre, norm = np.asarray(ext, float) / 2, np.linalg.norm(ext)
    tol = 1e-6 * norm  # f32 camera coordinates of a few |ext|
    th = np.tan(DEFAULT_HFOV / 2)
    for cam in cams:
        eye, fwd, right, upv = cam[0:3], cam[3:6], cam[6:9], cam[9:12]
        assert abs(np.linalg.norm(fwd) - 1) < 1e-6
        assert abs(fwd @ upv) < 1e-6 and abs(fwd @ right) < 1e-6 and abs(right @ upv) < 1e-6
        assert abs(np.linalg.norm(right) - th) < 1e-6 and abs(np.linalg.norm(upv) - th * H / W) < 1e-6
        # looks at the box centre, from 1.3 |ext| out and 0.5 |ext| up along the vertical
        d = centre - eye
        assert np.linalg.norm(np.cross(d, fwd)) < 4 * tol and d @ fwd > 0
        assert abs((eye - centre) @ up - 0.5 * norm) < 4 * tol
        out = (eye - centre) - ((eye - centre) @ up) * up
        assert abs(np.linalg.norm(out) - 1.3 * norm) < 4 * tol
        # up is the vertical, made perpendicular to forward
        assert upv @ up > 0 and abs(np.cross(fwd, up) @ upv) < 1e-6
    from atmonr_amd._lib import ANRError

    with pytest.raises(ANRError, match="no frames"):
        global_orbit_cameras(box, 0.0, 60, device="cpu")
    with pytest.raises(ANRError, match="vertical"):
        global_vertical(_Box((-5, -5, -5), (10, 10, 10)))


def _tool():
    spec = importlib.util.spec_from_file_location(
        "make_global_video_tool", os.path.join(ROOT, "tools", "make_global_video.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_tool_argument_parsing():
    ap = _tool().build_parser()
    a = ap.parse_args(["--voxels-filepath", "v.npy", "--sigma-filepath", "s.npy",
                       "--video-filepath", "o.mp4"])
    assert (a.voxels_filepath, a.sigma_filepath, a.video_filepath) == ("v.npy", "s.npy", "o.mp4")
    assert a.grid_res == 0.025 and a.grid_scale is None and a.render_band_idx == 2
    assert a.res == "640x480" and a.frame_rate == 60 and a.duration == 10.0
    assert tuple(a.absorb) == (0.1, 0.1, 0.1) and tuple(a.scatter) == (0.7, 0.7, 0.7)
    assert a.cutoff == 0.01 and a.light_source_dir is None and a.frames_dir == "_temp_frames"
    a = ap.parse_args(["--voxels-filepath", "v", "--sigma-filepath", "s", "--video-filepath", "o",
                       "--grid-res", "0.05", "--grid-scale", "2e-5", "--light-source-dir", "0",
                       "0", "2", "--res", "32x24", "--render-band-idx", "0"])
    assert a.grid_res == 0.05 and a.grid_scale == 2e-5 and a.light_source_dir == [0.0, 0.0, 2.0]
    for missing in ("--voxels-filepath", "--sigma-filepath", "--video-filepath"):
        argv = ["--voxels-filepath", "v", "--sigma-filepath", "s", "--video-filepath", "o"]
        k = argv.index(missing)
        with pytest.raises(SystemExit):
            ap.parse_args(argv[:k] + argv[k + 2:])
    # the options tools/make_video.py has and this tool keeps carry the same names and defaults
    spec = importlib.util.spec_from_file_location("make_video_tool",
                                                  os.path.join(ROOT, "tools", "make_video.py"))
    mv = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mv)
    dense = {x.dest: x.default for x in mv.build_parser()._actions}
    ours = {x.dest: x.default for x in ap._actions}
    for dest in ("video_filepath", "render_band_idx", "res", "frame_rate", "duration", "absorb",
                 "cutoff", "light_source_color", "scatter", "frames_dir"):
        assert ours[dest] == dense[dest], dest
    assert "extract_filepath" not in ours and "scene_scale" not in ours


def test_gpu_test_inputs_satisfy_their_conditions():
    """The yardstick alone keeps at least 98 % of the pixels of every half-emptied case, each
    case still sees the cloud, and the shell box is what the tests say it is."""
    for name in vc.CASES:
        voxels, values, cube, cams, H, W, P = sc.half_case(name)
        share = sc.half_compared(name).mean()
        print(f"{name}: {share:.2%} of the pixels compared, {voxels.shape[0]} of {cube.size} voxels")
        assert share >= 0.98
        assert 0.35 < voxels.shape[0] / cube.size < 0.65
        y = sc.half_reference(name)[0]
        assert y["rgba"][..., 3].max() > 0.05
    voxels, values = sc.shell_case()
    rel = voxels - voxels.min(axis=0)
    assert tuple(voxels.min(axis=0)) == sc.SHELL_LO and tuple(rel.max(axis=0) + 1) == sc.SHELL_EXT
    assert 0.08 < voxels.shape[0] / np.prod(sc.SHELL_EXT) < 0.15
    built = sc.np_build(voxels, values)
    live = sum(bin(int(w)).count("1") for w in built["coarse"])
    assert 0 < live < 9 * 3 * 3  # some bricks are dead: the brick level has something to skip
    # the restated lookup agrees with the yardstick's scalar one
    cube = sc.densify(*sc.build_case(), sc.BUILD_SCALE)
    pts = sc.lookup_points()[::97]
    want = sc.np_trilinear(cube, pts)
    for p, w in zip(pts, want):
        if np.isfinite(p).all() and np.all(np.abs(p) < 1e6):
            assert vc._sample(cube, [np.float32(x) for x in p], np.float32, vc._Pixel()) == w
