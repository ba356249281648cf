"""include_height without a GPU: the 4-D hash-grid level tables against the oracle, the
module layer's 4-input grid, and which combinations the Instant-NGP pipeline accepts.
No kernel launches."""

import numpy as np
import pytest
import torch

from oracle import ref_tcnn

PRIMES7 = [1, 2654435761, 805459861, 3674653429, 2097192037, 1434869437, 2165219737]


@pytest.mark.parametrize("cfg,total,sizes", [
    ((4, 16, 16, 1.3819, 19), 7_685_416, None),
    ((4, 4, 4, 1.5, 10), 256 + 3 * 1024, [256, 1024, 1024, 1024]),
])
def test_hashgrid_desc_4d_matches_oracle(cfg, total, sizes):
    from atmonr_amd import _lib

    d = _lib.hashgrid_desc(cfg[0], cfg[1], 2, cfg[2], cfg[3], cfg[4], allow_4d=True)
    offs, szs, res, scales, entries = ref_tcnn.grid_levels(*cfg)
    assert entries == total
    assert d.n_dims == 4 and d.n_params == 2 * entries
    assert list(d.offsets)[: cfg[1] + 1] == offs.tolist() + [entries]
    assert list(d.resolutions)[: cfg[1]] == res.tolist()
    assert list(d.scales)[: cfg[1]] == pytest.approx(scales.tolist(), rel=1e-7)
    if sizes is not None:
        assert szs.tolist() == sizes


def test_config3_grid_in_four_dimensions_has_the_three_kinds_of_level():
    """Levels 0-1 dense, 2-4 hashed with res^3 <= T (the stride loop runs through all four
    dimensions), 5-15 hashed with the loop stopping earlier; T * res stays below 2^32, the
    range over which the kernels' uint32 and uint64 stride arithmetic agree."""
    _, sizes, res, _, _ = ref_tcnn.grid_levels(4, 16, 16, 1.3819, 19)
    T = 1 << 19
    kinds = []
    for s, r in zip(sizes.tolist(), res.tolist()):
        assert s * r < 2 ** 32
        kinds.append("dense" if r ** 4 <= s else ("hash3" if r ** 3 <= T else "early"))
    assert kinds == ["dense"] * 2 + ["hash3"] * 3 + ["early"] * 11


def test_oracle_runs_in_four_dimensions(monkeypatch):
    monkeypatch.setattr(ref_tcnn, "PRIMES", np.array(PRIMES7[:4], dtype=np.uint32))
    cfg = (4, 4, 4, 1.5, 10)
    x = np.random.default_rng(0).random((50, 4)).astype(np.float32)
    x[:, 3] = x[:, 3] * 40 - 20
    for lvl in range(4):
        idx, wt = ref_tcnn.hashgrid_corners(x, cfg, lvl)
        assert idx.shape == (50, 16)
        np.testing.assert_allclose(wt.sum(1), 1.0, rtol=0, atol=1e-12)


def test_five_dimensions_still_rejected():
    from atmonr_amd import _lib
    from atmonr_amd.tcnn import Encoding

    with pytest.raises(_lib.ANRError, match="n_dims"):
        _lib.hashgrid_desc(5, 16, 2, 16, 1.38, 19, allow_4d=True)
    # anr_hashgrid_init itself keeps its 2-D / 3-D contract; 4-D is asked for by name
    with pytest.raises(_lib.ANRError, match="n_dims"):
        _lib.hashgrid_desc(4, 16, 2, 16, 1.3819, 19)
    assert _lib.load().anr_abi_version() == 5
    with pytest.raises(_lib.ANRError, match="input dims"):
        Encoding(5, {"otype": "HashGrid", "n_levels": 4})


def test_encoding_constructs_with_four_inputs():
    from atmonr_amd.tcnn import Encoding

    enc = Encoding(4, {"otype": "HashGrid", "n_levels": 16, "n_features_per_level": 2,
                       "log2_hashmap_size": 19, "base_resolution": 16,
                       "per_level_scale": 1.3819})
    assert enc.n_input_dims == 4 and enc.n_output_dims == 32
    assert enc.params.numel() == 2 * 7_685_416
    assert enc.hash_grids[0].desc.n_dims == 4


# ------------------------------------------------------------------ pipeline construction
class _Scene:
    """What Pipeline.__init__ reads from a dataset."""

    config = {"ray_origin_height": 2.0e4}
    scale = 1.0e5
    offset = torch.tensor([-2.5e6, -4.6e6, 3.6e6], dtype=torch.float64)
    max_i = 1.0

    def get_point_preprocessor(self, name):
        raise AssertionError("no preprocessor may be requested here")


def _cfg(**kw):
    from __graft_entry__ import _ingp_config

    cfg = _ingp_config(16)
    cfg.update(include_height=True, point_preprocessor=None)
    cfg.update(kw)
    return cfg


def test_pipeline_constructs_with_include_height():
    from atmonr_amd.pipelines.instant_ngp import InstantNGPPipeline

    pipe = InstantNGPPipeline(_cfg(), _Scene())
    assert pipe.pos_encoder.n_input_dims == 4
    assert pipe.pos_mlp.n_input_dims == 32
    p = pipe._prep_ngp
    assert (p.mode, p.ngp_remap, p.alt_compress) == (2, 1, 8.0)
    assert p.scale == 1.0e5 and list(p.offset) == [-2.5e6, -4.6e6, 3.6e6]
    assert p.ray_origin_height == 2.0e4
    # without the option: the 3-D grid, the raw points (mode 0) through the fused sampler
    pipe = InstantNGPPipeline(_cfg(include_height=False), _Scene())
    assert pipe.pos_encoder.n_input_dims == 3 and pipe._prep_ngp.mode == 0


def test_include_height_with_horizontal_preprocessor_trips_the_base_class():
    from atmonr_amd.pipelines.instant_ngp import InstantNGPPipeline

    with pytest.raises(AssertionError):
        InstantNGPPipeline(_cfg(point_preprocessor="horizontal"), _Scene())


def test_unsupported_combinations_raise_value_error():
    from atmonr_amd.pipelines.instant_ngp import InstantNGPPipeline

    with pytest.raises(ValueError, match="include_height"):
        InstantNGPPipeline(_cfg(), _Scene(), numerics="reference")
    with pytest.raises(ValueError, match="include_height"):
        InstantNGPPipeline(_cfg(numerics="reference"), _Scene())
    with pytest.raises(ValueError, match="include_height"):
        InstantNGPPipeline(_cfg(occupancy_grid={"resolution": 32}), _Scene())
    with pytest.raises(ValueError, match="include_height"):
        InstantNGPPipeline(_cfg(), _Scene(), occupancy=object())


def test_nerf_pipeline_keeps_refusing_and_says_why():
    from atmonr_amd.pipelines.nerf import NeRFPipeline

    cfg = {"type": "NeRF", "include_height": True, "point_preprocessor": None}
    with pytest.raises(NotImplementedError, match="backward into the sample positions"):
        NeRFPipeline(cfg, _Scene())
