"""The forward-only render without a GPU: anr_ingp_render is declared, exported and refuses
what it cannot take before any launch; ``render`` exists on both pipelines; render_rays
cuts a ray list into the right batches. No kernel runs."""

import ctypes
import os
import re

import pytest
import torch

from tests.conftest import ROOT

FAKE = 0x10000  # a non-null, 16-byte aligned address that is never dereferenced


def _descs(n_dims=3, dir_inputs=19):
    from atmonr_amd import _lib

    if n_dims == 3:
        grid = _lib.hashgrid_desc(3, 16, 2, 16, 1.3819, 19)
    else:
        grid = _lib.HashGridDesc()
        rc = _lib.load().anr_hashgrid_init_nd(ctypes.byref(grid), n_dims, 16, 2, 16, 1.3819, 19)
        assert rc == 0
    pos = _lib.mlp_desc(32, 16, 64, 1, False)
    dird = _lib.mlp_desc(dir_inputs, 4, 64, 2, False)
    return grid, pos, dird


def _call(grid, pos, dird, B=4, N=64, packed=FAKE, coords=FAKE, numerics=1, cmap=FAKE):
    from atmonr_amd import _lib

    lib = _lib.load()
    rc = lib.anr_ingp_render(ctypes.byref(grid), coords, FAKE, FAKE, B, N, FAKE, _lib.F16,
                             ctypes.byref(pos), ctypes.byref(dird), _lib.F16, packed, FAKE,
                             1.0, numerics, cmap, FAKE, FAKE, None)
    return rc, lib.anr_last_error().decode()


def test_symbol_is_declared_exported_and_bound():
    from atmonr_amd import _lib

    src = open(os.path.join(ROOT, "include", "anr.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert re.search(r"\banr_ingp_render\s*\(", src)
    assert "anr_ingp_render" in _lib.symbols()
    assert hasattr(_lib.load(), "anr_ingp_render")
    assert _lib.load().anr_abi_version() == 5
    assert (_lib.RENDER_BUILD, _lib.RENDER_REFERENCE) == (0, 1)
    for name, val in (("ANR_RENDER_BUILD", 0), ("ANR_RENDER_REFERENCE", 1)):
        assert re.search(rf"#define {name} {val}\b", src)


def test_zero_rays_is_a_no_op_success():
    grid, pos, dird = _descs()
    rc, _ = _call(grid, pos, dird, B=0, packed=None, coords=None, cmap=None)
    assert rc == 0


@pytest.mark.parametrize("case", ["n96", "n0", "grid4d", "multiband", "misaligned", "null_coords",
                                  "null_cmap", "numerics"])
def test_refusals_carry_a_message(case):
    """Every refusal comes back before a launch (the pointers are fake) with the entry's
    name and the reason in anr_last_error."""
    kw, want_rc, word = {}, -3, "unsupported"
    grid, pos, dird = _descs()
    if case == "n96":
        kw["N"] = 96
        word = "multiple of 64"
    elif case == "n0":
        kw["N"] = 0
        word = "multiple of 64"
    elif case == "grid4d":
        grid, pos, dird = _descs(n_dims=4)
        word = "3-D"
    elif case == "multiband":
        grid, pos, dird = _descs(dir_inputs=16)  # 20 - 16 = 4 density outputs
        word = "multi_band_extinction"
    elif case == "misaligned":
        kw["packed"] = FAKE + 8
        word = "16-byte aligned"
    elif case == "null_coords":
        kw["coords"] = None
        want_rc, word = -1, "null pointer"
    elif case == "null_cmap":
        kw["cmap"] = None
        want_rc, word = -1, "null pointer"
    else:
        kw["numerics"] = 2
        want_rc, word = -1, "numerics"
    rc, msg = _call(grid, pos, dird, **kw)
    assert rc == want_rc, (rc, msg)
    assert "anr_ingp_render" in msg and word in msg, msg


def test_render_exists_on_both_pipelines():
    import inspect

    from atmonr_amd.pipelines.instant_ngp import InstantNGPPipeline
    from atmonr_amd.pipelines.nerf import NeRFPipeline

    for cls in (InstantNGPPipeline, NeRFPipeline):
        sig = inspect.signature(cls.render)
        assert list(sig.parameters)[:5] == ["self", "ray_batch", "u", "random", "fused"]
        assert sig.parameters["random"].default is False
        assert sig.parameters["fused"].default == "auto"


class _StubRays:
    device = torch.device("cpu")

    def __init__(self, n):
        self.n = n

    def __len__(self):
        return self.n

    def __getbatch__(self, idx):
        return {"idx": idx.clone()}


class _StubPipeline:
    def __init__(self):
        self.calls = []

    def render(self, batch, **kw):
        idx = batch["idx"]
        self.calls.append((idx.tolist(), kw))
        maps = idx[:, None].float() * torch.tensor([1.0, 10.0, 100.0, 1000.0])
        return {"color_map_fine": maps, "color_map_atmo": maps + 0.25, "color_map_surf": -maps,
                "z_vals_fine": torch.zeros(idx.shape[0], 3)}


def test_render_rays_cuts_batches_in_order():
    from atmonr_amd.render import render_rays

    pipe = _StubPipeline()
    out = render_rays(pipe, _StubRays(40), batch_size=7, fused=False)
    assert [c[0] for c in pipe.calls] == [list(range(s, min(40, s + 7))) for s in range(0, 40, 7)]
    assert all(c[1] == {"fused": False} for c in pipe.calls)
    want = torch.arange(40)[:, None].float() * torch.tensor([1.0, 10.0, 100.0, 1000.0])
    assert sorted(out) == ["color_map_atmo", "color_map_fine", "color_map_surf"]
    assert torch.equal(out["color_map_fine"], want)
    assert torch.equal(out["color_map_atmo"], want + 0.25)
    assert torch.equal(out["color_map_surf"], -want)
    # a ray list: those rays, in that order
    pipe = _StubPipeline()
    idx = torch.tensor([31, 2, 2, 17, 39, 0, 5, 8, 9])
    out = render_rays(pipe, _StubRays(40), idx=idx, batch_size=4)
    assert [c[0] for c in pipe.calls] == [[31, 2, 2, 17], [39, 0, 5, 8], [9]]
    assert torch.equal(out["color_map_fine"][:, 0], idx.float())
