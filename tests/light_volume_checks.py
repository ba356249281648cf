"""Yardstick for the light-volume shadow mode (anr_volume_light, anr_volume_render_lit and their
sparse twins), in numpy on the CPU; it never imports the kernel or the package. It reuses the
marched yardstick's parts (tests/volume_checks.py: ``_sample``, ``_clip``, ``_Pixel``,
``MARGIN``, its cases and cameras) and restates only what the mode defines in include/anr.h.

``light`` restates tau one scalar operation at a time: per voxel with density > 0, the marched
shadow loop from the voxel's position as a plain sum, no early termination. ``render`` restates
the lit march: the marched primary loop with the shadow march replaced by the weighted mean of
tau over the corners with density > 0. Every value is held in ``dtype``: ``float64`` is the
yardstick, ``float32`` the arm that sizes tolerances.

Margins. A voxel's margin is the smallest distance of its tau's decisions to their thresholds:
``s1 / shadow_step`` to the nearest integer, and ``|ds - cutoff| / cutoff`` for every density
test (not with ``cutoff = 0``, where the test decides nothing). A pixel's margin is the marched
yardstick's for the decisions that remain (the step counts of the primary ray, the primary
density tests, the pixel's termination tests), and it also takes the margin of every voxel
whose tau it used with ``ww > 0``. Pixels and voxels below ``MARGIN`` are left out of the
comparisons with the kernel; tests/test_light_volume_cpu.py caps their share.

Cases. With the light along an axis every voxel's ``s1 / shadow_step`` lands exactly on an
integer, which excludes the voxel (and was measured to exclude 34-100 % of the pixels of
``cutoff0``). The yardstick comparisons therefore use oblique lights: ``cutoff`` and
``channels`` as they stand, and two cases made here from ``cutoff0``'s cube and cameras. The
default, axis-aligned light is covered by the exact tests of tests/test_light_volume_gpu.py.
Parity with vdb_render: unpinned.
"""

from __future__ import annotations

import functools

import numpy as np

from tests import volume_checks as vc

FLAGS = ("density_skip", "pixel_terminate", "miss")
CASES = ("cutoff", "channels", "cutoff0_oblique", "default_oblique")


@functools.lru_cache(maxsize=None)
def case(name: str):
    """(density, cameras (F, 12) f32, H, W, Params) of a named case."""
    if name in ("cutoff", "channels"):
        return vc.case(name)
    den, cams, H, W, _ = vc.case("cutoff0")
    if name == "cutoff0_oblique":
        return den, cams, H, W, vc.Params(cutoff=0.0, light_dir=vc._unit((0.45, 0.8, -0.4)),
                                          shadow_step=0.6, light_gain=0.1)
    if name == "default_oblique":
        return den, cams, H, W, vc.Params(light_dir=vc._unit((0.3, 0.9, 0.2)), shadow_step=0.7)
    raise KeyError(name)


def _consts(P: vc.Params, dt):
    f32 = lambda x: dt(np.float32(x))  # noqa: E731  (parameters reach the kernel as f32)
    return ([f32(x) for x in P.light_dir], f32(P.shadow_step), f32(P.light_gain), f32(P.cutoff))


def voxel_tau(den, v, P: vc.Params, dt):
    """(tau as dt, margin) of voxel ``v`` = (i, j, k)."""
    light, ss, gain_k, cutoff = _consts(P, dt)
    px = vc._Pixel()
    p = [dt(v[a]) for a in range(3)]
    tau, one = dt(0), dt(1)
    hit, _, s1 = vc._clip(den.shape, p, light, dt)
    if not hit:
        return tau, px.margin
    px.decide(vc._nearest_int_distance(s1 / ss))
    q = 1
    while True:
        s = dt(q) * ss
        q += 1
        if not s <= s1:
            break
        ds = vc._sample(den, [p[a] + s * light[a] for a in range(3)], dt, px)
        if cutoff > 0:
            px.decide(abs(ds - cutoff) / cutoff)
        if ds < cutoff:
            continue
        tau = tau + ds * ss / (one + s * gain_k)
    return tau, px.margin


def light(den, P: vc.Params, dtype=np.float64) -> dict:
    """tau (nx, ny, nz) f64 array of the ``dtype`` results, 0 where the density is not > 0,
    and margin (nx, ny, nz), inf there."""
    dt = np.dtype(dtype).type
    den = np.asarray(den, dtype=np.float32)
    out = {"tau": np.zeros(den.shape), "margin": np.full(den.shape, np.inf)}
    with np.errstate(over="ignore", under="ignore"):
        for v in np.ndindex(*den.shape):
            if den[v] > 0:
                tau, margin = voxel_tau(den, v, P, dt)
                out["tau"][v], out["margin"][v] = float(tau), margin
    return out


def _tau_hat(den, lit, p, dt, px):
    """The weighted mean of tau over the corners of p with density > 0, x outermost, z
    innermost, the low corner first; the pixel takes the margin of every corner it used."""
    f = [np.floor(p[a]) for a in range(3)]
    w = [p[a] - f[a] for a in range(3)]
    i, j, k = (int(f[a]) for a in range(3))
    n = den.shape
    one = dt(1)
    num, dn = dt(0), dt(0)
    for a in (0, 1):
        for b in (0, 1):
            for c in (0, 1):
                ww = ((w[0] if a else one - w[0]) * (w[1] if b else one - w[1])) * \
                    (w[2] if c else one - w[2])
                ci, cj, ck = i + a, j + b, k + c
                if not (0 <= ci < n[0] and 0 <= cj < n[1] and 0 <= ck < n[2]):
                    continue
                if not den[ci, cj, ck] > 0:
                    continue
                num = num + ww * dt(lit["tau"][ci, cj, ck])
                dn = dn + ww
                if ww > 0:
                    px.decide(lit["margin"][ci, cj, ck])
    return num / dn if dn > 0 else dt(0)


def render_pixel(den, lit, cam, col, row, H, W, P: vc.Params, dt):
    """(rgba[4] as dt, _Pixel) of one pixel of the lit march; ``lit``: light(den, P, dt)."""
    px = vc._Pixel()
    with np.errstate(over="ignore", under="ignore"):
        return _render_pixel(den, lit, cam, col, row, H, W, P, dt, px), px


def _render_pixel(den, lit, cam, col, row, H, W, P, dt, px):
    cam = [dt(x) for x in np.asarray(cam, dtype=np.float32)]
    eye, fwd, right, up = cam[0:3], cam[3:6], cam[6:9], cam[9:12]
    f32 = lambda x: dt(np.float32(x))  # noqa: E731
    absorb, scatter = [f32(x) for x in P.absorb], [f32(x) for x in P.scatter]
    lcol = [f32(x) for x in P.light_color]
    ps, cutoff = f32(P.primary_step), f32(P.cutoff)
    one, zero = dt(1), dt(0)
    ext, albedo = [], []
    for c in range(3):
        tot = absorb[c] + scatter[c]
        ext.append(-tot)
        albedo.append(zero if tot == 0 else lcol[c] * scatter[c] / tot)

    u = dt(2) * (dt(col) + dt(0.5)) / dt(W) - one
    v = dt(2) * (dt(row) + dt(0.5)) / dt(H) - one
    d = [fwd[a] + u * right[a] - v * up[a] for a in range(3)]
    ln = np.sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2])
    d = [d[a] / ln for a in range(3)]

    hit, t0, t1 = vc._clip(den.shape, eye, d, dt)
    if not hit:
        px.flags[2] = True
        return [zero] * 4
    if t0 > 0:
        px.decide(vc._nearest_int_distance(t0 / ps))
    else:
        t0 = zero
    tstart = ps * np.ceil(t0 / ps)
    px.decide(vc._nearest_int_distance((t1 - tstart) / ps))

    T, L = [one] * 3, [zero] * 3
    n = 0
    while True:
        t = tstart + dt(n) * ps
        n += 1
        if not t <= t1:
            break
        p = [eye[a] + t * d[a] for a in range(3)]
        dens = vc._sample(den, p, dt, px)
        if cutoff > 0:
            px.decide(abs(dens - cutoff) / cutoff)
        if dens < cutoff:
            px.flags[0] = True
            continue
        th = _tau_hat(den, lit, p, dt, px)
        sT = [np.exp(ext[c] * th) for c in range(3)]
        for c in range(3):
            dT = np.exp(ext[c] * dens * ps)
            L[c] = L[c] + albedo[c] * sT[c] * T[c] * (one - dT)
            T[c] = T[c] * dT
        t2 = T[0] * T[0] + T[1] * T[1] + T[2] * T[2]
        if cutoff > 0:
            px.decide(abs(t2 - cutoff) / cutoff)
        if t2 < cutoff:
            px.flags[1] = True
            break
    return [L[0], L[1], L[2], one - (T[0] + T[1] + T[2]) / dt(3)]


def render(den, cams, H: int, W: int, P: vc.Params, dtype=np.float64, lit=None) -> dict:
    """All pixels of all cameras: rgba (F, H, W, 4) f64 array of the ``dtype`` results, flags
    (F, H, W, 3) bool in FLAGS order, margin (F, H, W), and the light volume used
    (``light(den, P, dtype)`` unless given) under "light"."""
    dt = np.dtype(dtype).type
    den = np.asarray(den, dtype=np.float32)
    cams = np.asarray(cams, dtype=np.float32).reshape(-1, 12)
    lit = light(den, P, dtype) if lit is None else lit
    F = cams.shape[0]
    out = {"rgba": np.zeros((F, H, W, 4)), "flags": np.zeros((F, H, W, 3), dtype=bool),
           "margin": np.zeros((F, H, W)), "light": lit}
    for f in range(F):
        for row in range(H):
            for col in range(W):
                rgba, px = render_pixel(den, lit, cams[f], col, row, H, W, P, dt)
                out["rgba"][f, row, col] = [float(x) for x in rgba]
                out["flags"][f, row, col] = px.flags[:3]
                out["margin"][f, row, col] = px.margin
    return out


def _freeze(o):
    for a in o.values():
        if isinstance(a, dict):
            _freeze(a)
        else:
            a.setflags(write=False)


@functools.lru_cache(maxsize=None)
def reference(name: str):
    """(f64 yardstick, f32 arm) of a named case, computed once per process and left unchanged."""
    den, cams, H, W, P = case(name)
    out = render(den, cams, H, W, P, np.float64), render(den, cams, H, W, P, np.float32)
    for o in out:
        _freeze(o)
    return out


@functools.lru_cache(maxsize=None)
def marched_alpha(name: str) -> np.ndarray:
    """(F, H, W) f64: the alpha channel of the marched f64 yardstick (volume_checks) of the
    case, which the lit march must reproduce: it does not depend on the shadows."""
    if name in vc.CASES:
        return vc.reference(name)[0]["rgba"][..., 3]
    den, cams, H, W, P = case(name)
    a = vc.render(den, cams, H, W, P, np.float64)["rgba"][..., 3]
    a.setflags(write=False)
    return a


def compared_pixels(name: str) -> np.ndarray:
    """(F, H, W) bool: the pixels a comparison with the yardstick uses (margin >= MARGIN)."""
    return reference(name)[0]["margin"] >= vc.MARGIN


def compared_voxels(name: str) -> np.ndarray:
    """(nx, ny, nz) bool: the voxels whose tau is compared (density > 0, margin >= MARGIN)."""
    den = case(name)[0]
    return (den > 0) & (reference(name)[0]["light"]["margin"] >= vc.MARGIN)


def _bound(got, y, arm, keep):
    e_got = np.abs(np.asarray(got, dtype=np.float64) - y)[keep].max(axis=0)
    e_arm = np.abs(arm - y)[keep].max(axis=0)
    return e_got, e_arm, np.maximum(4.0 * e_arm, 2.0 ** -20 * np.abs(y)[keep].max(axis=0))


def errors(name: str, got) -> tuple:
    """(e_got, e_arm, bound) per channel, each (4,): the largest absolute difference to the
    f64 yardstick on the compared pixels, of ``got`` (F, H, W, 4) and of the f32 arm, and the
    bound max(4 e_arm, 2^-20 max|yardstick|) (the convention of tests/test_volume_gpu.py)."""
    y, arm = reference(name)
    return _bound(got, y["rgba"], arm["rgba"], compared_pixels(name))


def tau_errors(name: str, got) -> tuple:
    """The same three scalars for a tau cube ``got`` (nx, ny, nz) on the compared voxels."""
    y, arm = reference(name)
    return _bound(got, y["light"]["tau"], arm["light"]["tau"], compared_voxels(name))
