"""multi_band_extinction without a GPU: which dir networks the native field accepts, the
parameter count of the 16-wide first dir layer, and what the pipeline constructs."""

import ctypes

import pytest
import torch

import __graft_entry__ as ge


def _cfg(num_bands=4, n=64, width=64, nhd=2):
    cfg = ge._ingp_config(n)
    cfg.update(multi_band_extinction=True, num_bands=num_bands)
    cfg["instant_ngp"]["network"]["n_neurons"] = width
    cfg["instant_ngp"]["rgb_network"].update(n_neurons=width, n_hidden_layers=nhd)
    return cfg


@pytest.fixture(scope="module")
def scene():
    from atmonr_amd.datasets.synthetic import SyntheticHARP2Dataset

    return SyntheticHARP2Dataset(n_views=4, img_size=8, device=torch.device("cpu"), seed=0)


@pytest.mark.parametrize("width", [32, 64])
@pytest.mark.parametrize("nhd", [1, 2])
def test_field_supported_dir_inputs(width, nhd):
    from atmonr_amd import _lib

    lib = _lib.load()
    pos = _lib.mlp_desc(32, 16, width, 1, False)
    for n_in in range(14, 22):
        dir_ = _lib.mlp_desc(n_in, 4, width, nhd, False)
        want = 1 if 16 <= n_in <= 19 else 0
        assert lib.anr_ingp_field_supported(ctypes.byref(pos), ctypes.byref(dir_)) == want, n_in
        if want:
            assert dir_.n_input_padded == (16 if n_in == 16 else 32)
            # the fragments keep the K = 32 MFMA shape: one packed size for every S
            assert (lib.anr_ingp_field_packed_size(ctypes.byref(pos), ctypes.byref(dir_)) ==
                    lib.anr_ingp_field_packed_size(
                        ctypes.byref(pos), ctypes.byref(_lib.mlp_desc(19, 4, width, nhd, False))))
        else:
            assert lib.anr_ingp_field_packed_size(ctypes.byref(pos), ctypes.byref(dir_)) == 0
    # a descriptor whose padding is not tcnn's is refused
    bad = _lib.mlp_desc(16, 4, width, nhd, False)
    bad.n_input_padded = 32
    assert lib.anr_ingp_field_supported(ctypes.byref(pos), ctypes.byref(bad)) == 0
    # other widths / depths stay refused for every S
    assert lib.anr_ingp_field_supported(ctypes.byref(pos), ctypes.byref(
        _lib.mlp_desc(16, 4, width, 3, False))) == 0


@pytest.mark.parametrize("width", [32, 64])
@pytest.mark.parametrize("nhd", [1, 2])
def test_dir_network_parameter_count(width, nhd):
    from atmonr_amd import _lib

    lib = _lib.load()
    n4 = lib.anr_mlp_n_params(ctypes.byref(_lib.mlp_desc(16, 4, width, nhd, False)))
    assert n4 == 16 * width + (nhd - 1) * width * width + 16 * width
    for n_in in (17, 18, 19):
        n = lib.anr_mlp_n_params(ctypes.byref(_lib.mlp_desc(n_in, 4, width, nhd, False)))
        assert n == 32 * width + (nhd - 1) * width * width + 16 * width


def test_pipeline_constructs_fused(scene):
    from atmonr_amd.pipelines.instant_ngp import InstantNGPPipeline

    p = InstantNGPPipeline(_cfg(), scene)
    assert p.num_density_outputs == 4
    assert p.dir_encoder.n_input_dims == 15
    assert p.dir_mlp.n_input_dims == 16
    assert p.fused is True
    # bf16 field MLPs over f16 tables: fused too (they have no other path)
    b = InstantNGPPipeline(_cfg(), scene, mlp_dtype=torch.bfloat16)
    assert b.fused is True and b.pos_mlp.dtype == torch.bfloat16
    # two and three bands: the 32-wide first dir layer
    for nb in (2, 3):
        q = InstantNGPPipeline(_cfg(num_bands=nb), scene)
        assert q.fused is True and q.dir_mlp.n_input_dims == 20 - nb
        assert q.dir_mlp.desc.n_input_padded == 32


def test_pipeline_keeps_the_unfused_path_elsewhere(scene):
    from atmonr_amd.pipelines.instant_ngp import InstantNGPPipeline

    assert InstantNGPPipeline(_cfg(), scene, dtype=torch.float32).fused is False
    assert InstantNGPPipeline(_cfg(), scene, fused=False).fused is False
    assert InstantNGPPipeline(_cfg(num_bands=5), scene).fused is False
    # a field the native kernels do not take (three dir hidden layers)
    assert InstantNGPPipeline(_cfg(nhd=3), scene).fused is False
    with pytest.raises(ValueError):
        InstantNGPPipeline(_cfg(), scene, dtype=torch.float32, mlp_dtype=torch.bfloat16)
    # one density output: as ever
    cfg = ge._ingp_config(64)
    assert InstantNGPPipeline(cfg, scene).fused is True


def test_reference_numerics_still_refuse_multiband(scene):
    from atmonr_amd.pipelines.instant_ngp import InstantNGPPipeline

    with pytest.raises(ValueError):
        InstantNGPPipeline(_cfg(), scene, numerics="reference")
