"""Yardstick for a voxel traversal, on the CPU in f64; it never imports the kernel.

For a segment ``u -> end`` in a grid of unit voxels and a margin ``eps``, the f64 slab test
is run on every voxel of the segment's index bounding box grown by one, twice:

* ``sure``: voxels whose cube shrunk by ``eps`` on every side the segment hits;
* ``maybe``: voxels whose cube grown by ``eps`` on every side it hits.

A correct traversal ``got`` satisfies ``sure <= got <= maybe``: only voxels that the segment
grazes within ``eps`` of a face, an edge or a corner are free. The slab test's own rounding
(a few ulp of the coordinates) is far below any ``eps`` used with it.
"""

from __future__ import annotations

import numpy as np


def _hits(u, d, lo, hi):
    """Slab test of the segment u + t d, t in [0, 1], against boxes lo..hi (n, 3)."""
    tmin = np.zeros(lo.shape[0])
    tmax = np.ones(lo.shape[0])
    ok = np.ones(lo.shape[0], dtype=bool)
    for a in range(3):
        if d[a] == 0.0:
            ok &= (lo[:, a] <= u[a]) & (u[a] <= hi[:, a])
            continue
        t1, t2 = (lo[:, a] - u[a]) / d[a], (hi[:, a] - u[a]) / d[a]
        tmin = np.maximum(tmin, np.minimum(t1, t2))
        tmax = np.minimum(tmax, np.maximum(t1, t2))
    return ok & (tmin <= tmax)


def segment_voxels(u, end, eps: float):
    """(sure, maybe): two sets of (i, j, k) int tuples for one segment."""
    u = np.asarray(u, dtype=np.float64)
    end = np.asarray(end, dtype=np.float64)
    fu, fe = np.floor(u), np.floor(end)
    lo = (np.minimum(fu, fe) - 1).astype(np.int64)
    hi = (np.maximum(fu, fe) + 1).astype(np.int64)
    axes = [np.arange(lo[a], hi[a] + 1) for a in range(3)]
    vox = np.stack(np.meshgrid(*axes, indexing="ij"), axis=-1).reshape(-1, 3)
    v = vox.astype(np.float64)
    d = end - u
    sure = vox[_hits(u, d, v + eps, v + 1.0 - eps)]
    maybe = vox[_hits(u, d, v - eps, v + 1.0 + eps)]
    return set(map(tuple, sure.tolist())), set(map(tuple, maybe.tolist()))


def union_voxels(us, ends, eps: float):
    """Unions of ``sure`` and of ``maybe`` over the segments us[r] -> ends[r]."""
    sure, maybe = set(), set()
    for u, e in zip(np.asarray(us, dtype=np.float64), np.asarray(ends, dtype=np.float64)):
        s, m = segment_voxels(u, e, eps)
        sure |= s
        maybe |= m
    return sure, maybe


def as_set(voxels) -> set:
    """(n, 3) integer array or tensor -> set of tuples."""
    arr = voxels.cpu().numpy() if hasattr(voxels, "cpu") else np.asarray(voxels)
    return set(map(tuple, arr.reshape(-1, 3).astype(np.int64).tolist()))


def sandwich(got, sure, maybe) -> str:
    """Empty when ``sure <= got <= maybe``; otherwise what is missing or spurious."""
    missing, spurious = sorted(sure - got), sorted(got - maybe)
    if not missing and not spurious:
        return ""
    return f"{len(missing)} missing {missing[:5]}, {len(spurious)} spurious {spurious[:5]}"
