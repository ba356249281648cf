"""Pins tests/voxel_checks.py, the yardstick of the voxel-traversal tests, on hand-written
segments (CPU, f64; the helper never touches the kernel)."""

from tests import voxel_checks as vc

EPS = 1e-6


def test_axis_parallel_segment():
    sure, maybe = vc.segment_voxels((0.5, 0.5, 0.5), (2.5, 0.5, 0.5), EPS)
    assert sure == {(0, 0, 0), (1, 0, 0), (2, 0, 0)}
    assert maybe == sure


def test_zero_length_segment_is_one_voxel():
    sure, maybe = vc.segment_voxels((1.5, -2.5, 3.25), (1.5, -2.5, 3.25), EPS)
    assert sure == maybe == {(1, -3, 3)}


def test_diagonal_through_lattice_corners():
    sure, maybe = vc.segment_voxels((0.5, 0.5, 0.5), (3.5, 3.5, 3.5), EPS)
    assert sure == {(n, n, n) for n in range(4)}
    # at every corner (c, c, c) the seven other cubes around it are grazed, not entered
    graze = {(a, b, c) for n in range(3) for a in (n, n + 1) for b in (n, n + 1)
             for c in (n, n + 1)}
    assert maybe == graze and sure < maybe
    assert (1, 0, 0) in maybe and (1, 0, 0) not in sure
    assert (2, 0, 0) not in maybe


def test_negative_coordinates():
    sure, maybe = vc.segment_voxels((-0.5, -0.5, -0.5), (-2.5, -1.25, -0.5), EPS)
    # x crosses -1 at t = 0.25 (y = -0.6875), y crosses -1 at t = 2/3 (x = -1.83), x -2 at 0.75
    assert sure == maybe == {(-1, -1, -1), (-2, -1, -1), (-2, -2, -1), (-3, -2, -1)}
    # floor, not truncation: a segment inside (-1, 0)^3 is voxel -1, not 0
    assert vc.segment_voxels((-0.25, -0.5, -0.75), (-0.5, -0.25, -0.5), EPS)[0] == {(-1, -1, -1)}


def test_start_on_a_boundary_is_free_only_there():
    sure, maybe = vc.segment_voxels((2.0, 0.5, 0.5), (0.5, 0.5, 0.5), EPS)
    assert sure == {(1, 0, 0), (0, 0, 0)}
    assert maybe == sure | {(2, 0, 0)}


def test_unions_and_sandwich_report():
    us, ends = [(0.5, 0.5, 0.5), (0.5, 0.5, 0.5)], [(2.5, 0.5, 0.5), (0.5, 2.5, 0.5)]
    sure, maybe = vc.union_voxels(us, ends, EPS)
    assert sure == maybe == {(0, 0, 0), (1, 0, 0), (2, 0, 0), (0, 1, 0), (0, 2, 0)}
    assert vc.sandwich(set(sure), sure, maybe) == ""
    assert "1 missing" in vc.sandwich(sure - {(1, 0, 0)}, sure, maybe)
    assert "1 spurious" in vc.sandwich(sure | {(5, 5, 5)}, sure, maybe)
    import numpy as np

    assert vc.as_set(np.array([[1, 2, 3], [1, 2, 3], [-1, 0, 4]], dtype=np.int32)) == \
        {(1, 2, 3), (-1, 0, 4)}
