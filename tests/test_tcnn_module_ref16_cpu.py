"""atmonr_amd.tcnn's ``loss_scale`` and InstantNGPPipeline(fused=False,
numerics="reference") without a GPU: defaults, tcnn.reference_numerics(), the refused
constructor arguments, and what the unfused reference pipeline constructs and refuses."""

import pytest
import torch

import __graft_entry__ as ge


def _grid_cfg():
    return ge._ingp_config(64)["instant_ngp"]["encoding"]


def _net_cfg():
    return ge._ingp_config(64)["instant_ngp"]["network"]


@pytest.fixture(scope="module")
def scene():
    from atmonr_amd.datasets.synthetic import SyntheticHARP2Dataset

    return SyntheticHARP2Dataset(n_views=4, img_size=8, device=torch.device("cpu"), seed=0)


def test_defaults_unchanged():
    from atmonr_amd import tcnn

    assert tcnn.Encoding(3, _grid_cfg()).loss_scale is None
    assert tcnn.Network(32, 16, _net_cfg()).loss_scale is None


def test_reference_numerics_sets_the_default():
    from atmonr_amd import tcnn

    try:
        tcnn.reference_numerics()
        assert tcnn.Encoding(3, _grid_cfg()).loss_scale == 128.0
        assert tcnn.Network(32, 16, _net_cfg()).loss_scale == 128.0
        # f32 modules (tinycudann: loss scale 1) and f32 outputs keep the build's backward
        assert tcnn.Encoding(3, _grid_cfg(), dtype=torch.float32).loss_scale is None
        assert tcnn.Network(32, 16, _net_cfg(), dtype=torch.float32).loss_scale is None
        assert tcnn.Network(32, 16, _net_cfg(), output_dtype=torch.float32).loss_scale is None
    finally:
        tcnn.reference_numerics(False)
    assert tcnn.Encoding(3, _grid_cfg()).loss_scale is None
    assert tcnn.Network(32, 16, _net_cfg()).loss_scale is None


def test_explicit_loss_scale():
    from atmonr_amd import tcnn
    from atmonr_amd._lib import ANRError

    assert tcnn.Encoding(3, _grid_cfg(), loss_scale=128.0).loss_scale == 128.0
    assert tcnn.Network(32, 16, _net_cfg(), loss_scale=64).loss_scale == 64.0
    for build in (
            lambda: tcnn.Encoding(3, _grid_cfg(), dtype=torch.float32, loss_scale=128.0),
            lambda: tcnn.Network(32, 16, _net_cfg(), dtype=torch.float32, loss_scale=128.0),
            lambda: tcnn.Encoding(3, _grid_cfg(), output_dtype=torch.float32, loss_scale=128.0),
            lambda: tcnn.Network(32, 16, _net_cfg(), output_dtype=torch.float32,
                                 loss_scale=128.0),
            lambda: tcnn.Network(32, 16, _net_cfg(), loss_scale=0.0),
            lambda: tcnn.Encoding(3, _grid_cfg(), loss_scale=-1.0)):
        with pytest.raises((ANRError, ValueError), match="loss_scale"):
            build()


def test_unfused_reference_pipeline_constructs(scene):
    from atmonr_amd.pipelines.instant_ngp import InstantNGPPipeline

    p = InstantNGPPipeline(ge._ingp_config(64), scene, fused=False, numerics="reference")
    assert p.fused is False and p.numerics == "reference"
    for m in p.modules():
        assert m.loss_scale == 128.0, m
        assert m.output_dtype == torch.float16
    assert p.surf_mlp.output_dtype == torch.float16


def test_pipeline_modules_ignore_the_bare_module_default(scene):
    """tcnn.reference_numerics() is for bare modules: a build-numerics pipeline constructed
    while it is on keeps the build's backward in every module."""
    from atmonr_amd import tcnn
    from atmonr_amd.pipelines.instant_ngp import InstantNGPPipeline

    try:
        tcnn.reference_numerics()
        for fused in (True, False):
            p = InstantNGPPipeline(ge._ingp_config(64), scene, fused=fused)
            assert all(m.loss_scale is None for m in p.modules())
        # the fused reference path: only the surface network runs the scaled backward itself
        p = InstantNGPPipeline(ge._ingp_config(64), scene, numerics="reference")
        assert [m.loss_scale for m in p.modules()] == [None] * 5 + [128.0]
    finally:
        tcnn.reference_numerics(False)


def test_unfused_reference_pipeline_still_refuses(scene):
    from atmonr_amd.pipelines.instant_ngp import InstantNGPPipeline

    kw = dict(fused=False, numerics="reference")
    with pytest.raises(ValueError):
        InstantNGPPipeline(ge._ingp_config(64), scene, dtype=torch.float32, **kw)
    with pytest.raises(ValueError):
        InstantNGPPipeline(ge._ingp_config(64), scene, mlp_dtype=torch.bfloat16, **kw)
    with pytest.raises(ValueError):
        InstantNGPPipeline(ge._ingp_config(64), scene, occupancy=object(), **kw)
    cfg = ge._ingp_config(64)
    cfg.update(include_height=True, point_preprocessor=None)
    with pytest.raises(ValueError):
        InstantNGPPipeline(cfg, scene, **kw)
    cfg = ge._ingp_config(64)
    cfg.update(multi_band_extinction=True, num_bands=4)
    with pytest.raises(ValueError):
        InstantNGPPipeline(cfg, scene, **kw)
