"""Writes tests/golden/voxel_traversal.npz: the reference's own ``voxel_traversal``
(src/atmonr/graphics_utils.py:80-147) and its spherical-frame helpers
(src/atmonr/geospatial/spherical.py:15-36) on the CPU.

    ATMONR_REF=<checkout of nasa/atmospheric-neural-rendering>/src \\
        python tools/gen_globalgrid_golden.py

The reference package ``atmonr`` is imported from ATMONR_REF at generation time only; the
fixture stores inputs and the reference's outputs, nothing of its source.

* Traversal: 256 f32 segments, ``u ~ U(-12, 12)^3``, ``end = u + U(-12, 12)^3`` (seed in the
  file), and per ray the reference's ``voxel_traversal(unique_only=True)``. Before writing,
  every ray's set is checked against the f64 slab yardstick (tests/voxel_checks.py) at
  ``eps = 1e-5``: ``sure <= reference <= maybe``, and for at least 90 % of the rays ``sure ==
  maybe``, so that there any correct traversal equals the reference's. No segments at large
  coordinates: there the reference's f32 accumulation leaves the true path now and then.
* Spherical helpers: 4,096 points at radius EARTH_RADIUS +- 30 km, in f32 and f64, through
  ``wgs_84_to_spherical``, ``spherical_to_wgs84`` and ``stretch_above_sea_level`` with 12 and
  1 / 12. Stretch 1 returned its input bit for bit in both precisions (asserted here), so
  its output is the stored input.
"""

from __future__ import annotations

import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SEED = 31
N_RAYS = 256
N_POINTS = 4096
EPS = 1e-5


def main() -> None:
    ref = os.environ.get("ATMONR_REF")
    if not ref or not os.path.isdir(os.path.join(ref, "atmonr")):
        sys.exit("set ATMONR_REF to the reference checkout's src directory")
    sys.path.insert(0, ref)
    from atmonr.geospatial import spherical as ref_sph  # the reference's
    from atmonr.graphics_utils import voxel_traversal  # the reference's

    from tests import voxel_checks

    gen = torch.Generator().manual_seed(SEED)
    u = (torch.rand(N_RAYS, 3, generator=gen) * 2 - 1) * 12
    end = u + (torch.rand(N_RAYS, 3, generator=gen) * 2 - 1) * 12
    assert u.dtype == torch.float32 and end.dtype == torch.float32
    rows, offsets, exact = [], [0], 0
    for r in range(N_RAYS):
        vox = voxel_traversal(u[r:r + 1].clone(), end[r:r + 1].clone(), unique_only=True)
        vox = np.unique(vox.numpy().astype(np.int32), axis=0)
        sure, maybe = voxel_checks.segment_voxels(u[r].double().numpy(), end[r].double().numpy(),
                                                  EPS)
        bad = voxel_checks.sandwich(voxel_checks.as_set(vox), sure, maybe)
        assert not bad, f"the reference leaves the sandwich on ray {r}: {bad}"
        exact += sure == maybe
        rows.append(vox)
        offsets.append(offsets[-1] + vox.shape[0])
    assert exact >= 0.9 * N_RAYS, f"only {exact} of {N_RAYS} rays have sure == maybe"

    out = {}
    dirs = torch.randn(N_POINTS, 3, generator=gen, dtype=torch.float64)
    dirs = dirs / torch.linalg.norm(dirs, dim=-1, keepdim=True)
    radius = ref_sph.EARTH_RADIUS + (torch.rand(N_POINTS, 1, generator=gen,
                                                dtype=torch.float64) * 2 - 1) * 30e3
    pts64 = dirs * radius
    for name, pts in (("f32", pts64.float()), ("f64", pts64)):
        out[f"to_spherical_{name}"] = ref_sph.wgs_84_to_spherical(pts.clone()).numpy()
        out[f"to_wgs84_{name}"] = ref_sph.spherical_to_wgs84(pts.clone()).numpy()
        out[f"stretch_12_{name}"] = ref_sph.stretch_above_sea_level(pts.clone(), 12).numpy()
        out[f"stretch_inv12_{name}"] = ref_sph.stretch_above_sea_level(pts.clone(), 1 / 12).numpy()
        assert torch.equal(ref_sph.stretch_above_sea_level(pts.clone(), 1), pts)
        assert all(v.dtype == pts.numpy().dtype for k, v in out.items() if k.endswith(name))
    path = os.path.join(ROOT, "tests", "golden", "voxel_traversal.npz")
    np.savez_compressed(
        path, seed=np.int64(SEED), eps=np.float64(EPS), u_f32=u.numpy(), end_f32=end.numpy(),
        ref_voxels=np.concatenate(rows), ref_offsets=np.asarray(offsets, dtype=np.int64),
        earth_radius=np.float64(ref_sph.EARTH_RADIUS), points_f64=pts64.numpy(), **out)
    print("wrote", path, os.path.getsize(path), "bytes;", offsets[-1], "reference voxels,",
          exact, "of", N_RAYS, "rays with sure == maybe")


if __name__ == "__main__":
    main()
