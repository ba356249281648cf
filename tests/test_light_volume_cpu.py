"""The light-volume shadow mode without a GPU: its yardstick (tests/light_volume_checks.py)
meets the conditions the GPU tests rely on, its entries are declared, exported and bound at
ABI 5 and refuse what they cannot take before any launch, and the host layer refuses CPU
tensors and unknown modes."""

import ctypes
import importlib.util
import os
import re

import numpy as np
import pytest
import torch

from tests import light_volume_checks as lc
from tests import volume_checks as vc
from tests.conftest import ROOT

FAKE = 0x10000  # a non-null, 16-byte aligned address that is never dereferenced
ENTRIES = ("anr_volume_light", "anr_volume_render_lit", "anr_sparse_volume_light",
           "anr_sparse_volume_render_lit")


# ------------------------------------------------------------------ the yardstick
def test_cases_are_the_issue_s():
    assert lc.CASES == ("cutoff", "channels", "cutoff0_oblique", "default_oblique")
    for name in ("cutoff", "channels"):
        assert lc.case(name) is vc.case(name)
    den0, cams0, H, W, _ = vc.case("cutoff0")
    den, cams, h, w, P = lc.case("cutoff0_oblique")
    assert den is den0 and cams is cams0 and (h, w) == (H, W) == (16, 24)
    assert P == vc.Params(cutoff=0.0, light_dir=vc._unit((0.45, 0.8, -0.4)), shadow_step=0.6,
                          light_gain=0.1)
    den, cams, h, w, P = lc.case("default_oblique")
    assert den is den0 and cams is cams0
    assert P == vc.Params(light_dir=vc._unit((0.3, 0.9, 0.2)), shadow_step=0.7)
    for name in lc.CASES:  # oblique: no light along an axis
        assert np.all(np.abs(lc.case(name)[4].light_dir) > 0.1)


@pytest.mark.parametrize("name", lc.CASES)
def test_gpu_case_inputs_satisfy_the_conditions(name):
    """By the f64 yardstick alone: at most 2 % of an image's pixels are excluded (a decision,
    their own or one of a voxel whose tau they used, within 1e-4 of its threshold); on the
    compared pixels the f32 arm takes the yardstick's branches; the alpha channel is the
    marched yardstick's exactly; tau is defined where the density is > 0 and nowhere else."""
    den, cams, H, W, P = lc.case(name)
    y, arm = lc.reference(name)
    excluded = ~lc.compared_pixels(name)
    for f in range(cams.shape[0]):
        assert excluded[f].mean() <= 0.02, (name, f, excluded[f].mean())
    keep = lc.compared_pixels(name)
    assert np.array_equal(arm["flags"][keep], y["flags"][keep])
    miss = y["flags"][..., 2]
    assert miss.any() and not miss.all()
    if P.cutoff > 0:
        assert y["flags"][..., 0][~miss].mean() >= 0.05  # the density test decides something
        if name != "default_oblique":  # strong coefficients: rays end early
            assert y["flags"][..., 1][~miss].mean() >= 0.10
    else:
        assert not y["flags"][..., :2].any()
    # A does not depend on the shadows
    assert np.array_equal(y["rgba"][..., 3], lc.marched_alpha(name))
    # the light volume
    tau, margin = y["light"]["tau"], y["light"]["margin"]
    assert np.all(tau[den <= 0] == 0.0) and np.all(np.isinf(margin[den <= 0]))
    # (a voxel under the lit face can have no shadow sample at or above the cutoff: tau 0)
    assert np.all(tau[den > 0] >= 0.0) and (tau[den > 0] > 0.0).mean() > 0.9
    assert 0.3 < tau.max() < 3.0
    voxels = lc.compared_voxels(name)
    assert voxels.sum() >= 0.98 * (den > 0).sum()
    # the arm is close but not equal, and the bounds are tight in absolute terms
    e_got, e_arm, bound = lc.errors(name, arm["rgba"])
    assert np.all(e_got == e_arm) and np.all(e_arm > 0) and np.all(bound < 1e-5)
    t_got, t_arm, t_bound = lc.tau_errors(name, arm["light"]["tau"])
    assert t_got == t_arm and 0 < t_arm and t_bound < 1e-5
    print(f"{name}: excluded {excluded.mean():.4f} e_arm {e_arm.tolist()} tau e_arm {t_arm}")


def test_the_lit_colours_differ_from_the_marched_ones():
    """The mode is another arithmetic, not a rounding of the marched one: on the per-voxel
    noise cube the RGB of the two f64 yardsticks differ by far more than any tolerance here,
    while staying the same picture."""
    y = lc.reference("channels")[0]["rgba"]
    m = vc.reference("channels")[0]["rgba"]
    diff = np.abs(y[..., :3] - m[..., :3]).max()
    assert 1e-3 < diff < 0.2, diff


def test_tau_is_the_marched_shadow_loop_without_termination():
    """On a voxel, with cutoff 0, exp(ext * tau) is the marched shadow transmittance up to
    rounding: the f64 product of the marched loop's factors against exp of the f64 sum."""
    den, _, _, _, P = lc.case("cutoff0_oblique")
    v = (3, 1, 2)
    tau, _ = lc.voxel_tau(den, v, P, np.float64)
    light = [np.float64(np.float32(x)) for x in P.light_dir]
    ss, gain = np.float64(np.float32(P.shadow_step)), np.float64(np.float32(P.light_gain))
    _, _, s1 = vc._clip(den.shape, [np.float64(x) for x in v], light, np.float64)
    prod, q = 1.0, 1
    while q * ss <= s1:
        s = q * ss
        ds = vc._sample(den, [v[a] + s * light[a] for a in range(3)], np.float64, vc._Pixel())
        prod *= np.exp(-0.8 * ds * ss / (1.0 + s * gain))
        q += 1
    assert q > 3 and abs(prod - np.exp(-0.8 * tau)) < 1e-14


# ------------------------------------------------------------------ the C ABI
def test_entries_are_declared_exported_and_bound():
    from atmonr_amd import _lib

    src = open(os.path.join(ROOT, "include", "anr.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name in ENTRIES:
        assert re.search(r"\b%s\s*\(" % name, code), name
        assert name in _lib.symbols() and hasattr(_lib.load(), name)
        assert name in src.split("#define ANR_ABI_VERSION")[0]  # listed under "added to ABI 5"
    assert _lib.load().anr_abi_version() == 5
    assert ctypes.sizeof(_lib.VolumeParams) == 64 and ctypes.sizeof(_lib.SparseVolumeDesc) == 56


def _desc(ni=70, nj=9, nk=11, row_pitch=96, n_values=100, cells=FAKE, values=FAKE, coarse=FAKE):
    from atmonr_amd import _lib

    d = _lib.SparseVolumeDesc()
    d.cells, d.values, d.coarse = cells, values, coarse
    d.ni, d.nj, d.nk, d.reserved, d.row_pitch, d.n_values = ni, nj, nk, 0, row_pitch, n_values
    return d


def _call(entry, den=FAKE, tau=FAKE, shape=(7, 5, 6), desc="default", skip=1, cams=FAKE, F=3,
          H=16, W=24, out=FAKE, params="default", **kw):
    """One of the four entries with fake pointers: (status, message)."""
    from atmonr_amd import _lib
    from atmonr_amd.video import VolumeRenderSettings

    lib = _lib.load()
    p = VolumeRenderSettings(**kw).params() if params == "default" else params
    p = ctypes.byref(p) if p is not None else None
    d = _desc() if desc == "default" else desc
    d = ctypes.byref(d) if d is not None else None
    if entry == "anr_volume_light":
        rc = lib.anr_volume_light(den, *shape, p, tau, None)
    elif entry == "anr_volume_render_lit":
        rc = lib.anr_volume_render_lit(den, tau, *shape, cams, F, H, W, p, out, None)
    elif entry == "anr_sparse_volume_light":
        rc = lib.anr_sparse_volume_light(d, skip, p, tau, None)
    else:
        rc = lib.anr_sparse_volume_render_lit(d, tau, skip, cams, F, H, W, p, out, None, None)
    return rc, lib.anr_last_error().decode()


PARAM_REFUSALS = {
    "null_params": (dict(params=None), "null pointer"),
    "zero_primary_step": (dict(primary_step=0.0), "steps must be positive"),
    "nan_shadow_step": (dict(shadow_step=float("nan")), "steps must be positive"),
    "tiny_shadow_step": (dict(shadow_step=1e-30), "steps too small"),
    "negative_absorb": (dict(absorb=(0.1, -0.1, 0.1)), "negative coefficient"),
    "negative_cutoff": (dict(cutoff=-0.01), "negative coefficient"),
    "negative_gain": (dict(light_gain=-0.2), "negative coefficient"),
    "light_not_unit": (dict(light_dir=(0.0, 1.01, 0.0)), "unit length"),
    "null_tau": (dict(tau=None), "null pointer"),
}


@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("case", sorted(PARAM_REFUSALS))
def test_every_entry_refuses_bad_params_and_a_null_tau(entry, case):
    kw, word = PARAM_REFUSALS[case]
    rc, msg = _call(entry, **kw)
    assert rc == -1 and entry + ":" in msg and word in msg, (rc, msg)


DENSE_REFUSALS = {
    "null_density": (dict(den=None), "null pointer"),
    "zero_extent": (dict(shape=(7, 0, 6)), "extents"),
    "negative_extent": (dict(shape=(-1, 5, 6)), "extents"),
    "cube_2_31_bytes": (dict(shape=(1024, 1024, 512)), "2^31 bytes"),
}
SPARSE_REFUSALS = {
    "null_volume": (dict(desc=None), "null pointer"),
    "null_cells": (dict(desc=_desc(cells=None)), "null pointer"),
    "null_values": (dict(desc=_desc(values=None)), "null pointer"),
    "null_coarse_with_skip": (dict(desc=_desc(coarse=None)), "null pointer"),
    "zero_extent": (dict(desc=_desc(nj=0)), "extents"),
    "pitch_below_ni": (dict(desc=_desc(row_pitch=64)), "row_pitch"),
    "words_2_31": (dict(desc=_desc(ni=1 << 12, nj=1 << 14, nk=1 << 12, row_pitch=1 << 12)),
                   "2^31 bitmap words"),
    "no_values": (dict(desc=_desc(n_values=0)), "n_values"),
    "values_2_31": (dict(desc=_desc(n_values=1 << 31)), "n_values"),
    "bad_skip": (dict(skip=2), "skip"),
}
IMAGE_REFUSALS = {
    "null_cameras": (dict(cams=None), "null pointer"),
    "null_output": (dict(out=None), "null pointer"),
    "negative_image": (dict(H=-1), "image size"),
    "image_side_2_24": (dict(W=1 << 24), "2^24"),
}


@pytest.mark.parametrize("case", sorted(DENSE_REFUSALS))
def test_dense_entries_refuse_what_the_render_refuses(case):
    kw, word = DENSE_REFUSALS[case]
    for entry in ENTRIES[:2]:
        rc, msg = _call(entry, **kw)
        assert rc == -1 and entry + ":" in msg and word in msg, (entry, rc, msg)


@pytest.mark.parametrize("case", sorted(SPARSE_REFUSALS))
def test_sparse_entries_refuse_what_the_render_refuses(case):
    kw, word = SPARSE_REFUSALS[case]
    for entry in ENTRIES[2:]:
        rc, msg = _call(entry, **kw)
        assert rc == -1 and entry + ":" in msg and word in msg, (entry, rc, msg)


@pytest.mark.parametrize("case", sorted(IMAGE_REFUSALS))
def test_lit_renders_refuse_what_the_renders_refuse(case):
    kw, word = IMAGE_REFUSALS[case]
    for entry in (ENTRIES[1], ENTRIES[3]):
        rc, msg = _call(entry, **kw)
        assert rc == -1 and entry + ":" in msg and word in msg, (entry, rc, msg)


def test_no_work_is_a_no_op_success():
    for entry in (ENTRIES[1], ENTRIES[3]):
        for kw in (dict(F=0), dict(H=0), dict(W=0)):
            rc, msg = _call(entry, den=None, tau=None, cams=None, out=None,
                            desc=_desc(cells=None, values=None, coarse=None), **kw)
            assert rc == 0, (entry, kw, msg)
    # without the brick level a null coarse passes; the call then fails on the null tau only
    for entry in ENTRIES[2:]:
        rc, msg = _call(entry, desc=_desc(coarse=None), skip=0, tau=None)
        assert rc == -1 and "null pointer" in msg
    # a box whose dense cube is refused (2.69 GB) is accepted up to the pointer check
    rc, msg = _call(ENTRIES[2], desc=_desc(973, 873, 791, 992, 78_300_000), tau=None)
    assert rc == -1 and "null pointer" in msg, msg


# ------------------------------------------------------------------ the host layer
def test_host_layer_refuses_cpu_tensors_and_unknown_modes():
    from atmonr_amd._lib import ANRError
    from atmonr_amd.sparse_volume import render_sparse_volume
    from atmonr_amd.video import (SHADOWS, LightVolume, VolumeRenderSettings, light_key,
                                  light_volume, make_video, render_volume)

    assert SHADOWS == ("marched", "light_volume")
    with pytest.raises(ANRError, match="GPU"):
        light_volume(torch.zeros(3, 3, 3))
    with pytest.raises(ANRError, match="GPU"):
        render_volume(torch.zeros(3, 3, 3), torch.zeros(1, 12), 8, 8, shadows="light_volume")
    for bad in ("light", "", None, "Marched"):
        with pytest.raises(ValueError, match="shadows"):
            render_volume(torch.zeros(3, 3, 3), torch.zeros(1, 12), 8, 8, shadows=bad)
        with pytest.raises(ValueError, match="shadows"):
            render_sparse_volume(None, torch.zeros(1, 12), 8, 8, shadows=bad)
        with pytest.raises(ValueError, match="shadows"):
            make_video("missing.npz", "nowhere", shadows=bad)
    # the key: what tau depends on besides the density, as f32 values
    a = VolumeRenderSettings()
    assert light_key(a) == (0.0, 1.0, 0.0, 3.0, float(np.float32(0.2)), float(np.float32(0.01)))
    assert light_key(VolumeRenderSettings(absorb=(1, 2, 3), primary_step=0.5)) == light_key(a)
    for kw in (dict(light_dir=(1.0, 0.0, 0.0)), dict(shadow_step=2.0), dict(light_gain=0.1),
               dict(cutoff=0.0)):
        assert light_key(VolumeRenderSettings(**kw)) != light_key(a), kw
    lv = LightVolume(torch.zeros(3, 4, 5), light_key(a))
    lv.check(a, (3, 4, 5), torch.device("cpu"))
    with pytest.raises(ANRError, match="other settings"):
        lv.check(VolumeRenderSettings(cutoff=0.0), (3, 4, 5), torch.device("cpu"))
    with pytest.raises(ANRError, match="shape"):
        lv.check(a, (3, 4, 6), torch.device("cpu"))


@pytest.mark.parametrize("tool", ["make_video", "make_global_video"])
def test_tools_take_the_shadows_option(tool):
    spec = importlib.util.spec_from_file_location(tool + "_tool",
                                                  os.path.join(ROOT, "tools", tool + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    parser = mod.build_parser()
    action = next(a for a in parser._actions if "--shadows" in a.option_strings)
    assert action.default == "marched" and tuple(action.choices) == ("marched", "light_volume")
