"""The light-volume shadow mode on the GPU (anr_volume_light, anr_volume_render_lit and the
sparse twins): tau and the lit frames against the f64 yardstick (tests/light_volume_checks.py),
and the exact properties the definition promises: the marched alpha, the tie with the marched
mode where every sample sits on a voxel, sparse equal to dense, frames independent.

Tolerance of the yardstick comparisons: the convention of tests/test_volume_gpu.py. Per
channel, on the pixels (voxels, for tau) the yardstick does not exclude, the largest absolute
difference to the f64 yardstick must be <= max(4 e_arm, 2^-20 max|yardstick|), e_arm being the
same distance of the yardstick's own float32 arm. Each case prints e_gpu and e_arm.
"""

import numpy as np
import pytest
import torch

from tests import light_volume_checks as lc
from tests import sparse_volume_checks as sc
from tests import volume_checks as vc

pytestmark = pytest.mark.gpu

ALL_CASES = lc.CASES + ("cutoff0", "down_odd")  # the last two: the default, axis-aligned light


def _t(a, dev):
    return torch.from_numpy(np.array(a)).to(dev)  # a copy: the inputs are read-only


def _settings(P: vc.Params):
    from atmonr_amd.video import VolumeRenderSettings

    return VolumeRenderSettings(**{k: getattr(P, k) for k in P.__dataclass_fields__})


def _case(name):
    return lc.case(name) if name in lc.CASES else vc.case(name)


def _dense(dev, den, cams, H, W, P, **kw):
    from atmonr_amd.video import render_volume

    out = render_volume(_t(den, dev), _t(cams, dev), W, H, _settings(P), **kw)
    torch.cuda.synchronize()
    return out


def _lit(dev, den, cams, H, W, P, **kw):
    return _dense(dev, den, cams, H, W, P, shadows="light_volume", **kw)


def _volume(dev, voxels, values):
    from atmonr_amd.sparse_volume import SparseVolume

    return SparseVolume.from_voxels(_t(voxels, dev), _t(values, dev))


def _sparse(dev, vol, cams, H, W, P, **kw):
    from atmonr_amd.sparse_volume import render_sparse_volume

    out = render_sparse_volume(vol, _t(cams, dev), W, H, _settings(P), **kw)
    torch.cuda.synchronize()
    return out


# ------------------------------------------------------------------ 1. the f64 yardstick
@pytest.mark.parametrize("name", lc.CASES)
def test_tau_and_frames_against_the_f64_yardstick(dev, name):
    from atmonr_amd.video import light_volume

    den, cams, H, W, P = lc.case(name)
    light = light_volume(_t(den, dev), _settings(P))
    tau = light.tau.cpu().numpy()
    assert tau.shape == den.shape and np.isfinite(tau).all()
    assert np.all(tau[den <= 0] == 0.0)
    t_gpu, t_arm, t_bound = lc.tau_errors(name, tau)
    print(f"{name}: tau e_gpu {t_gpu} e_arm {t_arm} bound {t_bound} compared "
          f"{int(lc.compared_voxels(name).sum())} of {int((den > 0).sum())} voxels")
    assert t_gpu <= t_bound, (name, t_gpu, t_bound)

    got = _lit(dev, den, cams, H, W, P, light=light).cpu().numpy()
    assert got.shape == (cams.shape[0], H, W, 4) and np.isfinite(got).all()
    e_gpu, e_arm, bound = lc.errors(name, got)
    keep = lc.compared_pixels(name)
    print(f"{name}: e_gpu {e_gpu.tolist()} e_arm {e_arm.tolist()} bound {bound.tolist()} "
          f"compared {int(keep.sum())} of {keep.size} pixels")
    assert np.all(e_gpu <= bound), (name, e_gpu, bound)
    miss = lc.reference(name)[0]["flags"][..., 2]
    assert np.all(got[miss] == 0.0)
    # a light volume built inside the call gives the same frames
    assert np.array_equal(_lit(dev, den, cams, H, W, P).cpu().numpy(), got)


# ------------------------------------------------------------------ 2. the marched alpha
@pytest.mark.parametrize("name", ALL_CASES)
def test_alpha_is_the_marched_frame_s_bit_for_bit(dev, name):
    den, cams, H, W, P = _case(name)
    marched = _dense(dev, den, cams, H, W, P)
    lit = _lit(dev, den, cams, H, W, P)
    assert float(marched[..., 3].max()) > 0.05
    assert torch.equal(lit[..., 3], marched[..., 3])
    # the colours are the mode's own: the same picture, not the same numbers
    diff = float((lit[..., :3] - marched[..., :3]).abs().max())
    print(f"{name}: largest RGB difference to the marched mode {diff:.4f}")
    assert diff < 0.2
    if name in lc.CASES:
        assert diff > 1e-4


# ------------------------------------------------------------------ 3. the tie
TIE_K = 7


def test_tie_with_the_marched_mode_on_voxel_samples(dev):
    """A 1 x 1 image from the integer eye (3, 0, 8) straight down -z through the voxel column
    (3, 0, :) of cutoff0's cube, primary_step 1, cutoff 0: every sample sits on a voxel (or at
    z = 6 and z = -1, outside the array, where d = 0 contributes nothing), so tau_hat is that
    voxel's tau and its shadow loop is the marched one from the same point. The lit and the
    marched RGB then differ only by exp(ext * sum) against the product of exps. K = 7 is the
    largest number of shadow steps of a sample here (light unit(0.3, 0.9, 0.2), shadow_step
    0.7, from y = 0 to the face y = 5: s1 = 5 / 0.928 = 5.39 voxels, 7 steps of 0.7).
    Per step the marched product takes at most 3 roundings of the argument (|argument| < 1),
    one exp within an ulp and one product, the sum at most 2 roundings per term and one per
    addition before a single exp: (4 K + 8) 2^-24 relative, per channel."""
    den = vc.make_cube(11).copy()
    den[3, 0, :] = np.maximum(den[3, 0, :], np.float32(0.05))  # the column is all cloud
    P = vc.Params(absorb=(0.3, 0.5, 0.8), scatter=(1.0, 1.5, 2.0), cutoff=0.0,
                  light_dir=vc._unit((0.3, 0.9, 0.2)), shadow_step=0.7)
    cam = vc.look_at((3.0, 0.0, 8.0), (3.0, 0.0, 0.0), (0.0, 1.0, 0.0), 1, 1)[None]
    assert list(cam[0, 3:6]) == [0.0, 0.0, -1.0]
    # K, counted in f64 from the clip of the voxels' shadow rays
    light = [np.float64(np.float32(x)) for x in P.light_dir]
    steps = []
    for k in range(den.shape[2]):
        hit, _, s1 = vc._clip(den.shape, [np.float64(3), np.float64(0), np.float64(k)], light,
                              np.float64)
        assert hit
        steps.append(int(np.floor(s1 / np.float64(np.float32(P.shadow_step)))))
    assert max(steps) == TIE_K, steps
    marched = _dense(dev, den, cam, 1, 1, P).cpu().numpy()[0, 0, 0].astype(np.float64)
    lit = _lit(dev, den, cam, 1, 1, P).cpu().numpy()[0, 0, 0].astype(np.float64)
    assert marched[3] == lit[3] and marched[3] > 0.5 and np.all(marched[:3] > 0.01)
    rel = np.abs(lit[:3] - marched[:3]) / marched[:3]
    bound = (4 * TIE_K + 8) * 2.0 ** -24
    print(f"tie: K {TIE_K} relative difference {rel.tolist()} bound {bound}")
    assert np.all(rel <= bound), (rel, bound)


# ------------------------------------------------------------------ 4. sparse against dense
def _sparse_equals_dense(dev, vol, voxels, cube, cams, H, W, P):
    from atmonr_amd.video import light_volume

    dense_light = light_volume(_t(cube, dev), _settings(P))
    dense = _lit(dev, cube, cams, H, W, P, light=dense_light)
    assert float(dense[..., 3].max()) > 0.05 and float(dense[..., :3].max()) > 0.01
    rel = np.asarray(voxels, dtype=np.int64) - np.asarray(vol.lo)
    # the voxels of the volume in value order: k, then j, then i
    order = np.lexsort((rel[:, 0], rel[:, 1], rel[:, 2]))
    i, j, k = (_t(rel[order, a], dev) for a in range(3))
    want_tau = dense_light.tau[i, j, k]
    for skip in (True, False):
        vol._light = None  # build it anew with this skip
        light = vol.light(_settings(P), skip=skip)
        assert light.tau.shape == vol.values.shape
        assert torch.equal(light.tau, want_tau), skip
        assert torch.equal(_sparse(dev, vol, cams, H, W, P, skip=skip, shadows="light_volume",
                                   light=light), dense), skip
    # the light volume the volume builds and keeps itself
    assert torch.equal(_sparse(dev, vol, cams, H, W, P, shadows="light_volume"), dense)
    return dense


@pytest.mark.parametrize("name", vc.CASES)
def test_sparse_equals_dense_half_emptied(dev, name):
    voxels, values, cube, cams, H, W, P = sc.half_case(name)
    _sparse_equals_dense(dev, _volume(dev, voxels, values), voxels, cube, cams, H, W, P)


@pytest.mark.parametrize("P", [vc.Params(), vc.Params(cutoff=0.0, shadow_step=1.0),
                               vc.Params(light_dir=vc._unit((0.3, 0.9, 0.2)), shadow_step=0.7)],
                         ids=["defaults", "cutoff0_shadow1", "oblique"])
def test_sparse_equals_dense_shell(dev, P):
    """The shell box (a row pitch of 96, bricks that are dead): brick level on and off, with
    the counters, against the dense kernels on the densified cube."""
    voxels, values = sc.shell_case()
    perm = np.random.default_rng(4).permutation(voxels.shape[0])
    vol = _volume(dev, voxels[perm], values[perm])
    cams, H, W = sc.shell_cameras(), sc.SHELL_H, sc.SHELL_W
    dense = _sparse_equals_dense(dev, vol, voxels, sc.densify(voxels, values), cams, H, W, P)
    counters = torch.zeros(2, dtype=torch.int64, device=dev)
    on = _sparse(dev, vol, cams, H, W, P, shadows="light_volume", counters=counters)
    assert torch.equal(on, dense)
    samples, skipped = counters.tolist()
    assert 0 < skipped < samples
    # the lit march takes the primary samples alone: fewer than the marched mode's
    marched = torch.zeros(2, dtype=torch.int64, device=dev)
    _sparse(dev, vol, cams, H, W, P, counters=marched)
    assert samples < marched.tolist()[0]


# ------------------------------------------------------------------ 5. frames and chunking
def test_frames_are_independent(dev):
    from atmonr_amd.video import light_volume

    den, cams, H, W, P = lc.case("cutoff")
    light = light_volume(_t(den, dev), _settings(P))
    whole = _lit(dev, den, cams, H, W, P, light=light)
    for f in range(cams.shape[0]):
        assert torch.equal(_lit(dev, den, cams[f:f + 1], H, W, P, light=light)[0], whole[f]), f
    for budget in (H * W * 16, 1, 2 * H * W * 16):
        assert torch.equal(_lit(dev, den, cams, H, W, P, light=light, max_bytes=budget), whole)
    assert _lit(dev, den, cams[:0], H, W, P, light=light).shape == (0, H, W, 4)
    voxels, values, _, cams, H, W, P = sc.half_case("cutoff")
    vol = _volume(dev, voxels, values)
    whole = _sparse(dev, vol, cams, H, W, P, shadows="light_volume")
    for f in range(cams.shape[0]):
        one = _sparse(dev, vol, cams[f:f + 1], H, W, P, shadows="light_volume")
        assert torch.equal(one[0], whole[f]), f
    for budget in (H * W * 16, 1):
        assert torch.equal(_sparse(dev, vol, cams, H, W, P, shadows="light_volume",
                                   max_bytes=budget), whole)


# ------------------------------------------------------------------ 6. the makers and the key
def test_a_light_volume_of_other_settings_is_not_reused(dev, tmp_path, monkeypatch):
    from atmonr_amd import sparse_volume as sv
    from atmonr_amd import video
    from atmonr_amd._lib import ANRError

    den, cams, H, W, P = lc.case("default_oblique")
    a = _settings(P)
    b = _settings(vc.Params(light_dir=P.light_dir, shadow_step=0.7, light_gain=0.0))
    light_a = video.light_volume(_t(den, dev), a)
    with pytest.raises(ANRError, match="other settings"):
        video.render_volume(_t(den, dev), _t(cams, dev), W, H, b, shadows="light_volume",
                            light=light_a)
    with pytest.raises(ANRError, match="shape"):
        video.render_volume(_t(den[:-1], dev), _t(cams, dev), W, H, a, shadows="light_volume",
                            light=light_a)
    # the sparse volume keeps the last light volume, keyed by what it depends on
    voxels, values = sc.shell_case()
    vol = _volume(dev, voxels, values)
    la = vol.light(a)
    assert vol.light(a) is la
    assert vol.light(_settings(vc.Params(light_dir=P.light_dir, shadow_step=0.7,
                                         absorb=(0.5,) * 3))) is la  # absorb is not in the key
    lb = vol.light(b)
    assert lb is not la and lb.key != la.key and not torch.equal(lb.tau, la.tau)
    with pytest.raises(ANRError, match="other settings"):
        sv.render_sparse_volume(vol, _t(sc.shell_cameras(), dev), 32, 24, b,
                                shadows="light_volume", light=la)
    # the makers: one build per video, for the video's settings
    builds = []
    real = sv.SparseVolume.light

    def counting(self, settings=None, skip=True):
        fresh = self._light is None or self._light[0] != video.light_key(
            sv.global_settings(self) if settings is None else settings)
        builds.append(fresh)
        return real(self, settings, skip)

    monkeypatch.setattr(sv.SparseVolume, "light", counting)
    kw = dict(width=32, height=24, duration=1.0, frame_rate=4, max_bytes=1)
    res_b = sv.make_global_video(vol, tmp_path / "b", None, settings=b, shadows="light_volume",
                                 **kw)
    assert builds == [False]  # lb, still kept
    res_a = sv.make_global_video(vol, tmp_path / "a", None, settings=a, shadows="light_volume",
                                 **kw)
    assert builds == [False, True]  # rebuilt once for a, not once per frame
    with pytest.raises(ANRError, match="other settings"):
        sv.make_global_video(vol, tmp_path / "c", None, settings=a, shadows="light_volume",
                             light=lb, **kw)
    assert len(res_a["frames"]) == 4
    assert any(open(x, "rb").read() != open(y, "rb").read()
               for x, y in zip(res_a["frames"], res_b["frames"]))
    # the frames are those of the lit render under the same settings
    cams4 = sv.global_orbit_cameras(vol, 1.0, 4, 32, 24)
    first = sv.render_sparse_volume(vol, cams4[:1], 32, 24, a, shadows="light_volume")[0]
    video.write_ppm(tmp_path / "first.ppm", first)
    assert open(tmp_path / "first.ppm", "rb").read() == open(res_a["frames"][0], "rb").read()
    # the dense maker: one light volume for all frames, and the marched default is untouched
    rng = np.random.default_rng(2)
    ext = rng.uniform(0.0, 0.3, (6, 7, 5, 4)).astype(np.float32)
    np.savez(tmp_path / "extract.npz", extinction=ext)
    dense_builds = []
    real_lv = video.light_volume
    monkeypatch.setattr(video, "light_volume",
                        lambda *x, **k: dense_builds.append(1) or real_lv(*x, **k))
    lit = video.make_video(tmp_path / "extract.npz", tmp_path / "lit", None, device=dev,
                           shadows="light_volume", **kw)
    assert dense_builds == [1] and len(lit["frames"]) == 4
    plain = video.make_video(tmp_path / "extract.npz", tmp_path / "plain", None, device=dev, **kw)
    assert dense_builds == [1]
    cube = _t(video.volume_from_extract(ext), dev)
    cams4 = video.orbit_cameras(cube.shape, 1.0, 4, 32, 24, device=dev)
    for frames, mode in ((lit, "light_volume"), (plain, "marched")):
        first = video.render_volume(cube, cams4[:1], 32, 24, shadows=mode)[0]
        video.write_ppm(tmp_path / "first.ppm", first)
        assert open(tmp_path / "first.ppm", "rb").read() == open(frames["frames"][0], "rb").read()
