"""Numpy restatements and inputs for the sparse volume's tests (csrc/sparse_volume.hip); it never
imports the kernel or the package.

``np_build`` restates the structure include/anr.h documents: bitmap words (i fastest, row
pitch a multiple of 32), the rank of every word, the values in ascending bitmap order, and the
brick bits. ``densify`` is the cube the sparse march must reproduce; ``np_trilinear`` is D(p)
of that cube in float32 in the written order (z pairs, then y, then x, each a + w (b - a)).
The yardstick of the march itself stays tests/volume_checks.py.
"""

from __future__ import annotations

import functools

import numpy as np

from tests import volume_checks as vc

BRICK_LOG2 = 3


# ------------------------------------------------------------------ restatements
def scale_values(values, density_scale: float) -> np.ndarray:
    """f64 product, NaN -> 0, one rounding to f32."""
    v = np.asarray(values, dtype=np.float32).astype(np.float64) * float(density_scale)
    return np.nan_to_num(v, nan=0.0).astype(np.float32)


def np_build(voxels, values, density_scale: float = 1.0) -> dict:
    """lo, ext, row_pitch, bits (n_words,) uint32, rank (n_words,) int64, values (n,) f32 in
    bitmap order, coarse (words,) uint32."""
    voxels = np.asarray(voxels, dtype=np.int64)
    lo = voxels.min(axis=0)
    ext = voxels.max(axis=0) - lo + 1
    rel = voxels - lo
    ni, nj, nk = (int(e) for e in ext)
    pitch = (ni + 31) // 32 * 32
    key = (rel[:, 2] * nj + rel[:, 1]) * pitch + rel[:, 0]
    order = np.argsort(key, kind="stable")
    bits = np.zeros(pitch // 32 * nj * nk, dtype=np.uint32)
    np.bitwise_or.at(bits, key >> 5, (np.uint32(1) << (key & 31).astype(np.uint32)))
    pop = np.array([bin(int(w)).count("1") for w in bits], dtype=np.int64)
    rank = np.cumsum(pop) - pop
    nb = [(int(e) >> BRICK_LOG2) + 1 for e in ext]
    coarse = np.zeros((nb[0] * nb[1] * nb[2] + 31) // 32, dtype=np.uint32)
    for d in np.ndindex(2, 2, 2):
        b = (rel - np.asarray(d) + 1) >> BRICK_LOG2
        brick = (b[:, 2] * nb[1] + b[:, 1]) * nb[0] + b[:, 0]
        np.bitwise_or.at(coarse, brick >> 5, np.uint32(1) << (brick & 31).astype(np.uint32))
    return {"lo": tuple(int(v) for v in lo), "ext": (ni, nj, nk), "row_pitch": pitch,
            "bits": bits, "rank": rank, "values": scale_values(values, density_scale)[order],
            "coarse": coarse, "popcount": int(pop.sum())}


def densify(voxels, values, density_scale: float = 1.0) -> np.ndarray:
    """(ni, nj, nk) f32, z fastest, zeros where no voxel is: anr_volume_render's cube."""
    voxels = np.asarray(voxels, dtype=np.int64)
    rel = voxels - voxels.min(axis=0)
    den = np.zeros(tuple(rel.max(axis=0) + 1), dtype=np.float32)
    den[rel[:, 0], rel[:, 1], rel[:, 2]] = scale_values(values, density_scale)
    return den


def np_trilinear(den, pts) -> np.ndarray:
    """D(p) of the cube ``den`` at (P, 3) f32 points, every operation in f32."""
    den = np.asarray(den, dtype=np.float32)
    pts = np.asarray(pts, dtype=np.float32)
    n = np.asarray(den.shape)
    with np.errstate(invalid="ignore"):
        f = np.floor(pts)
        ok = np.all((f >= -1) & (f <= (n - 1).astype(np.float32)), axis=1)
    out = np.zeros(pts.shape[0], dtype=np.float32)
    p, f = pts[ok], f[ok]
    w = p - f
    idx = f.astype(np.int64) + 1  # into the cube padded by one zero voxel on every side
    pad = np.pad(den, 1)
    i, j, k = idx[:, 0], idx[:, 1], idx[:, 2]
    wx, wy, wz = w[:, 0], w[:, 1], w[:, 2]

    def lerp(a, b, t):
        return a + t * (b - a)

    c00 = lerp(pad[i, j, k], pad[i, j, k + 1], wz)
    c01 = lerp(pad[i, j + 1, k], pad[i, j + 1, k + 1], wz)
    c10 = lerp(pad[i + 1, j, k], pad[i + 1, j, k + 1], wz)
    c11 = lerp(pad[i + 1, j + 1, k], pad[i + 1, j + 1, k + 1], wz)
    res = lerp(lerp(c00, c01, wy), lerp(c10, c11, wy), wx)
    assert res.dtype == np.float32
    out[ok] = res
    return out


# ------------------------------------------------------------------ the build case
# lo = (-37, 4090, -5), ext = (70, 9, 11): a row pitch of 96, three words per row, the last one
# part-filled (bits 0..5). About 30 % present. Forced: row (j, k) = (2, 3) holds exactly bits 0,
# 31, 32, 63, 64 and 69; word 1 of row (4, 5) is full; row (0, 0) is empty.
BUILD_LO = (-37, 4090, -5)
BUILD_EXT = (70, 9, 11)
BUILD_SCALE = 1594.25
EDGE_ROW, FULL_ROW, EMPTY_ROW = (2, 3), (4, 5), (0, 0)
EDGE_BITS = (0, 31, 32, 63, 64, 69)


@functools.lru_cache(maxsize=None)
def build_case():
    """(voxels (n, 3) int32 grid indices in bitmap order, values (n,) f32 with one NaN)."""
    ni, nj, nk = BUILD_EXT
    rng = np.random.default_rng(3)
    present = rng.random((nk, nj, ni)) < 0.3
    present[EDGE_ROW[1], EDGE_ROW[0], :] = False
    present[EDGE_ROW[1], EDGE_ROW[0], list(EDGE_BITS)] = True
    present[FULL_ROW[1], FULL_ROW[0], 32:64] = True
    present[EMPTY_ROW[1], EMPTY_ROW[0], :] = False
    k, j, i = np.nonzero(present)
    voxels = (np.stack([i, j, k], axis=1) + np.asarray(BUILD_LO)).astype(np.int32)
    values = rng.uniform(0.0, 2e-4, voxels.shape[0]).astype(np.float32)
    values[17] = np.nan
    for a in (voxels, values):
        a.setflags(write=False)
    return voxels, values


def shuffled(seed: int):
    voxels, values = build_case()
    perm = np.random.default_rng(seed).permutation(voxels.shape[0])
    return np.ascontiguousarray(voxels[perm]), np.ascontiguousarray(values[perm])


def lookup_points() -> np.ndarray:
    """(P, 3) f32 box-relative points of the lookup test on the build case's box."""
    ni, nj, nk = BUILD_EXT
    pitch = (ni + 31) // 32 * 32
    rng = np.random.default_rng(5)
    g = np.stack(np.meshgrid(np.arange(ni), np.arange(nj), np.arange(nk), indexing="ij"), -1)
    pts = [g.reshape(-1, 3).astype(np.float64)]                      # all voxel centres
    pts.append(rng.uniform(-1.0, 1.0, (4096, 3)) * 0.5 * np.asarray(BUILD_EXT) +
               0.5 * np.asarray(BUILD_EXT))                          # interior (and the rim)
    for a, n in enumerate(BUILD_EXT):                                # every face
        for x in (-1.0, -0.5, n - 1.0, n - 0.5, float(n)):
            p = rng.uniform(-1.0, np.asarray(BUILD_EXT, dtype=np.float64), (256, 3))
            p[:, a] = x
            pts.append(p)
    p = rng.uniform(-1.0, np.asarray(BUILD_EXT, dtype=np.float64), (2048, 3))
    p[:, 0] = rng.uniform(ni - 1.0, pitch, 2048)                     # the pad bits of a row
    pts.append(p)
    q = np.stack(np.meshgrid(np.arange(ni - 1, pitch + 1), np.arange(nj), np.arange(nk),
                             indexing="ij"), -1).reshape(-1, 3).astype(np.float64)
    pts.append(q)                                                    # and on the lattice
    pts.append(q + (0.5, 0.25, 0.75))
    far = np.array([[np.nan, 1, 1], [1, np.nan, 1], [1, 1, np.nan], [1e9, 1, 1], [1, -1e9, 1],
                    [1, 1, 3e38], [np.inf, 1, 1], [-np.inf, 2, 2], [-1.001, 1, 1],
                    [1, nj + 0.001, 1], [2 ** 31, 1, 1], [-2.0 ** 31, 1, 1]])
    pts.append(far)
    return np.concatenate(pts).astype(np.float32)


# ------------------------------------------------------------------ half-emptied standard cases
HALF_LO = (5, -3, 100)


@functools.lru_cache(maxsize=None)
def half_case(name: str):
    """volume_checks.case(name) with the voxels where default_rng(7).random(shape) < 0.5 made
    absent: (voxels (n, 3) int32 at HALF_LO, values (n,) f32, the densified cube, cameras, H, W,
    Params)."""
    den, cams, H, W, P = vc.case(name)
    absent = np.random.default_rng(7).random(den.shape) < 0.5
    i, j, k = np.nonzero(~absent)
    voxels = (np.stack([i, j, k], axis=1) + np.asarray(HALF_LO)).astype(np.int32)
    values = den[i, j, k].astype(np.float32)
    cube = densify(voxels, values)
    assert cube.shape == den.shape  # the present voxels reach every face of the cube
    for a in (voxels, values, cube):
        a.setflags(write=False)
    return voxels, values, cube, cams, H, W, P


@functools.lru_cache(maxsize=None)
def half_reference(name: str):
    """(f64 yardstick, f32 arm) of the half-emptied case, computed once per process."""
    _, _, cube, cams, H, W, P = half_case(name)
    out = vc.render(cube, cams, H, W, P, np.float64), vc.render(cube, cams, H, W, P, np.float32)
    for o in out:
        for a in o.values():
            a.setflags(write=False)
    return out


def half_compared(name: str) -> np.ndarray:
    return half_reference(name)[0]["margin"] >= vc.MARGIN


def half_errors(name: str, got) -> tuple:
    """volume_checks.errors for the half-emptied case: (e_got, e_arm, bound) per channel."""
    y, arm = half_reference(name)
    keep = half_compared(name)
    got = np.asarray(got, dtype=np.float64)
    e_got = np.abs(got - y["rgba"])[keep].max(axis=0)
    e_arm = np.abs(arm["rgba"] - y["rgba"])[keep].max(axis=0)
    bound = np.maximum(4.0 * e_arm, 2.0 ** -20 * np.abs(y["rgba"])[keep].max(axis=0))
    return e_got, e_arm, bound


# ------------------------------------------------------------------ the shell box
# A (70, 20, 19) box holding a thin shell | |v - c| - R | < 1.5 about a centre outside it: the
# shape of a global-grid extract, 12.7 % occupied. The shell runs from y = 0 at the x faces up
# through the top face, so the present voxels span the whole box.
SHELL_EXT = (70, 20, 19)
SHELL_LO = (-35, 6000, -9)
SHELL_CENTRE = (34.5, -15.0, 9.0)
SHELL_RADIUS = 37.5
SHELL_H, SHELL_W = 24, 32


@functools.lru_cache(maxsize=None)
def shell_case():
    """(voxels (n, 3) int32 at SHELL_LO, values (n,) f32 in [0.1, 0.3])."""
    g = np.stack(np.meshgrid(*(np.arange(n) for n in SHELL_EXT), indexing="ij"), -1)
    r = np.linalg.norm(g - np.asarray(SHELL_CENTRE), axis=-1)
    i, j, k = np.nonzero(np.abs(r - SHELL_RADIUS) < 1.5)
    voxels = (np.stack([i, j, k], axis=1) + np.asarray(SHELL_LO)).astype(np.int32)
    values = np.random.default_rng(9).uniform(0.1, 0.3, voxels.shape[0]).astype(np.float32)
    for a in (voxels, values):
        a.setflags(write=False)
    return voxels, values


def shell_cameras() -> np.ndarray:
    """Three orbit poses of the script's orbit around the box and one eye inside it."""
    H, W = SHELL_H, SHELL_W
    orbit = [vc.orbit_pose(SHELL_EXT, frac, H, W) for frac in (0.05, 0.4, 0.77)]
    inside = vc.look_at((20.3, 9.6, 8.2), (60.0, 14.0, 11.0), (0.0, 1.0, 0.0), H, W)
    return np.stack(orbit + [inside])
