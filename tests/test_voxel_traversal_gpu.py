"""The exact voxel traversal (csrc/voxels.hip, atmonr_amd.graphics_utils.voxel_traversal) on
the GPU, against the f64 slab yardstick of tests/voxel_checks.py and against the reference's
own traversal (tests/golden/voxel_traversal.npz, tools/gen_globalgrid_golden.py).

``EPS = 1e-6`` for the kernel's own sandwich: f64 at |x| <= 2^13 has an ulp of 9e-13 and the
crossing times are a few operations deep, so 1e-6 leaves six orders of margin. Only voxels
that a segment grazes within EPS are free; everything else must match.
"""

import numpy as np
import pytest
import torch

from tests import voxel_checks as vc
from tests.conftest import golden

pytestmark = pytest.mark.gpu

EPS = 1e-6


def _segments(seed, base, spread, n=512):
    rng = np.random.default_rng(seed)
    u = base + rng.uniform(-spread, spread, size=(n, 3))
    return u, u + rng.uniform(-spread, spread, size=(n, 3))


def _special():
    rays = [
        ((1.5, 2.5, 3.5), (1.5, 2.5, 3.5)),                 # zero length
        ((-0.25, -7.5, 2.0), (-0.25, -7.5, 2.0)),           # zero length on a boundary
        ((0.5, 0.5, 0.5), (7.5, 0.5, 0.5)),                 # parallel to x (d = 0 on y, z)
        ((0.5, 6.5, 0.5), (0.5, -4.5, 0.5)),                # parallel to y, downwards
        ((-2.5, 0.5, -3.5), (-2.5, 0.5, 5.5)),              # parallel to z
        ((40.5, 0.5, 0.5), (-40.5, 0.5, 0.5)),              # x, downwards, across three words
        ((2.0, 3.0, 1.0), (-1.5, 5.25, 3.5)),               # starts on integer boundaries
        ((2.0, 0.5, 0.5), (0.5, 0.5, 0.5)),                 # on a boundary, leaving it downwards
        ((-3.0, -3.0, -3.0), (1.0, 2.0, 4.0)),              # integer start and end
        ((0.5, 0.5, 0.5), (3.5, 3.5, 3.5)),                 # the corner diagonal
        ((3.5, 3.5, 0.5), (0.5, 0.5, 3.5)),                 # a corner diagonal, mixed signs
        ((0.3, 0.4, 0.2), (3000.7, 2.6, 1.9)),              # long and thin: ~94 words of a row
    ]
    a = np.asarray(rays, dtype=np.float64)
    return a[:, 0], a[:, 1]


SETS = {
    "near0": lambda: _segments(1, 0.0, 12.0),
    "at4100": lambda: _segments(2, 4100.0, 14.0),
    "at-3000": lambda: _segments(3, -3000.0, 10.0),
    "special": _special,
}


@pytest.fixture(scope="module")
def rays():
    """name -> (u, end, union of sure, union of maybe); computed once, never modified."""
    out = {}
    for name, make in SETS.items():
        u, end = make()
        out[name] = (u, end) + vc.union_voxels(u, end, EPS)
    return out


def _traverse(u, end, dev, **kw):
    from atmonr_amd.graphics_utils import voxel_traversal

    return voxel_traversal(torch.as_tensor(u, device=dev), torch.as_tensor(end, device=dev), **kw)


def _check(got, sure, maybe, what):
    assert got.dtype == torch.int32 and got.dim() == 2 and got.shape[1] == 3
    bad = vc.sandwich(vc.as_set(got), sure, maybe)
    assert not bad, f"{what}: {bad}"
    assert len(vc.as_set(got)) == got.shape[0], f"{what}: duplicates"


# ------------------------------------------------------------------ 1. the sandwich
@pytest.mark.parametrize("name", list(SETS))
def test_sandwich_all_rays_in_one_call(rays, dev, name):
    u, end, sure, maybe = rays[name]
    _check(_traverse(u, end, dev), sure, maybe, name)
    # f32 inputs are widened: the same segments as their f64 values
    if name == "near0":
        u32, e32 = u.astype(np.float32), end.astype(np.float32)
        s32, m32 = vc.union_voxels(u32[:64], e32[:64], EPS)
        _check(_traverse(u32[:64], e32[:64], dev), s32, m32, "near0 f32")


@pytest.mark.parametrize("R", [1, 63, 257])
def test_sandwich_ray_counts(rays, dev, R):
    u, end = rays["near0"][:2]
    sure, maybe = vc.union_voxels(u[:R], end[:R], EPS)
    _check(_traverse(u[:R], end[:R], dev), sure, maybe, f"R={R}")


def test_sandwich_one_ray_per_call(rays, dev):
    picks = [("special", r) for r in range(len(rays["special"][0]))]
    picks += [(n, r) for n in ("near0", "at4100", "at-3000") for r in range(7)]
    assert len(picks) >= 32
    for name, r in picks:
        u, end = rays[name][0][r:r + 1], rays[name][1][r:r + 1]
        sure, maybe = vc.segment_voxels(u[0], end[0], EPS)
        _check(_traverse(u, end, dev), sure, maybe, f"{name}[{r}]")


def test_unique_only_false_and_empty(rays, dev):
    u, end = rays["near0"][0][:63], rays["near0"][1][:63]
    assert torch.equal(_traverse(u, end, dev), _traverse(u, end, dev, unique_only=False))
    none = _traverse(np.zeros((0, 3)), np.zeros((0, 3)), dev)
    assert none.shape == (0, 3) and none.dtype == torch.int32


# ------------------------------------------------------------------ 2. order, determinism
def _popcount(words):
    w = words.to(torch.int64) & 0xFFFFFFFF
    return int(sum(((w >> b) & 1).sum() for b in range(32)).item())


def _bitmap(u, end, dev, shrink=None):
    from atmonr_amd.graphics_utils import VoxelBitmap

    ut, et = torch.as_tensor(u, device=dev), torch.as_tensor(end, device=dev)
    lo, hi = VoxelBitmap.bounds(ut, et)
    if shrink is not None:
        hi[shrink] -= 1
    return VoxelBitmap(lo, hi, dev), ut, et


def test_order_popcount_determinism_permutation_chunks(rays, dev):
    u, end = rays["near0"][:2]
    bm, ut, et = _bitmap(u, end, dev)
    bm.add(ut, et)
    got = bm.voxels()
    assert got.shape[0] == _popcount(bm.words)
    # ascending in bitmap order: k slowest, i fastest, a row row_pitch bits long
    rel = got.to(torch.int64) - torch.tensor(bm.lo, device=dev)
    assert bool((rel >= 0).all()) and bool((rel < torch.tensor(bm.ext, device=dev)).all())
    key = (rel[:, 2] * bm.ext[1] + rel[:, 1]) * bm.row_pitch + rel[:, 0]
    assert bool((key[1:] > key[:-1]).all())
    assert bm.row_pitch % 32 == 0 and bm.skipped_rays() == 0
    # a second run, and the convenience wrapper
    assert torch.equal(got, _traverse(u, end, dev))
    # without the load-before-atomic shortcut
    bm2, _, _ = _bitmap(u, end, dev)
    bm2.add(ut, et, shortcut=False)
    assert torch.equal(bm2.words, bm.words)
    # a random permutation of the rays
    perm = np.random.default_rng(9).permutation(u.shape[0])
    assert torch.equal(got, _traverse(u[perm], end[perm], dev))
    # two chunks into one bitmap
    bm3, _, _ = _bitmap(u, end, dev)
    bm3.add(ut[:200], et[:200])
    bm3.add(ut[200:], et[200:])
    assert torch.equal(bm3.words, bm.words) and torch.equal(bm3.voxels(), got)


def test_non_finite_endpoints_are_skipped(rays, dev):
    u, end = rays["near0"][0][:63].copy(), rays["near0"][1][:63].copy()
    want = _traverse(u, end, dev)
    u2 = np.concatenate([u, [[0.5, np.nan, 0.5], [1.5, 1.5, 1.5]]])
    e2 = np.concatenate([end, [[2.5, 0.5, 0.5], [np.inf, 1.5, 1.5]]])
    bm, ut, et = _bitmap(u2, e2, dev)
    bm.add(ut, et)
    assert bm.skipped_rays() == 2
    assert torch.equal(bm.voxels(), want)
    only = _traverse(u2[63:], e2[63:], dev)
    assert only.shape == (0, 3)


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_box_too_small_raises(rays, dev, axis):
    from atmonr_amd._lib import ANRError

    u, end = rays["near0"][:2]
    bm, ut, et = _bitmap(u, end, dev, shrink=axis)
    bm.add(ut, et)
    with pytest.raises(ANRError, match="leave the box"):
        bm.voxels()
    assert int(bm.counters[1].item()) > 0


# ------------------------------------------------------------------ 3. the reference
def test_against_the_reference_traversal(dev):
    g = golden("voxel_traversal.npz")
    eps = float(g["eps"])
    assert eps == 1e-5
    u, end = g["u_f32"], g["end_f32"]
    assert u.dtype == np.float32 and u.shape == (256, 3)
    off, ref = g["ref_offsets"], g["ref_voxels"]
    equal = 0
    for r in range(u.shape[0]):
        got = vc.as_set(_traverse(u[r:r + 1], end[r:r + 1], dev))
        want = vc.as_set(ref[off[r]:off[r + 1]])
        sure, maybe = vc.segment_voxels(u[r].astype(np.float64), end[r].astype(np.float64), eps)
        assert (got ^ want) <= (maybe - sure), (r, sorted(got ^ want))
        equal += got == want
    assert equal >= 0.9 * u.shape[0], equal
    # all rays in one call: the union of the reference's sets, up to grazing voxels
    sure, maybe = vc.union_voxels(u, end, eps)
    allv = vc.as_set(_traverse(u, end, dev))
    assert (allv ^ vc.as_set(ref)) <= (maybe - sure)


# ------------------------------------------------------------------ 4. the bitmap limit
def test_max_bitmap_bytes(rays, dev):
    u, end = rays["special"][:2]
    with pytest.raises(ValueError, match="max_bitmap_bytes"):
        _traverse(u, end, dev, max_bitmap_bytes=1024)
    assert _traverse(u, end, dev, max_bitmap_bytes=1 << 20).shape[0] > 3000
