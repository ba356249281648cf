"""Spherical-Earth frame of the global-grid extract -- the names and semantics of
src/atmonr/geospatial/spherical.py:12-36.

The WGS-84 ellipsoid is squeezed onto a sphere of ``EARTH_RADIUS`` (z scaled by A / B, then
everything by EARTH_RADIUS / A), and points above that sphere can be moved radially so that
their height above it is multiplied by a stretch factor. Unlike the reference's, the
functions here are out of place (the inputs are not modified), keep the input's dtype,
build no masked copies and take any leading shape ``(..., 3)``. The operations and their
order are the reference's, so f64 results agree with it bit for bit on one device.
"""

from __future__ import annotations

import torch

from .wgs_84 import A, B

EARTH_RADIUS = 6.378e6  # meters


def wgs_84_to_spherical(xyz: torch.Tensor) -> torch.Tensor:
    """WGS-84 Cartesian (..., 3) -> spherical-Earth Cartesian (spherical.py:15-18)."""
    z = xyz[..., 2:] * A / B
    return torch.cat([xyz[..., :2], z], dim=-1) * EARTH_RADIUS / A


def spherical_to_wgs84(xyz: torch.Tensor) -> torch.Tensor:
    """Inverse of :func:`wgs_84_to_spherical` (spherical.py:21-24)."""
    out = xyz * A / EARTH_RADIUS
    return torch.cat([out[..., :2], out[..., 2:] * (B / A)], dim=-1)


def stretch_above_sea_level(xyz: torch.Tensor, stretch: float) -> torch.Tensor:
    """Points with radius r > EARTH_RADIUS move to radius (r - EARTH_RADIUS) * stretch +
    EARTH_RADIUS along their own direction; points at or below the sphere are returned
    unchanged (spherical.py:27-36). ``1 / stretch`` undoes ``stretch``."""
    radii = torch.linalg.norm(xyz, dim=-1)
    above = radii > EARTH_RADIUS
    factor = ((radii - EARTH_RADIUS) * stretch + EARTH_RADIUS) / radii
    return torch.where(above[..., None], xyz * factor[..., None], xyz)
