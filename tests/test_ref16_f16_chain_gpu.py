"""Reference numerics with f16 interchange between the field kernels and the f16 composite
(ANR_REF_F16_IO, default on): the field forward writes sigma / colour as f16
(anr_ingp_field_fwd_h), the composite reads and saves them as they are, its f16 gradients
go to the field backward as they are (anr_ingp_field_bwd_ref16_rows_h), and the composite
backward parks its two scratch values as one 4-byte pair per sample. Every value is
rounded to f16 at the same point from the same f32 value as with f32 interchange, so the
results are the same: bit for bit wherever no f32 atomics are involved."""

import ctypes

import numpy as np
import pytest
import torch

import __graft_entry__ as ge
from oracle import ref_f16

pytestmark = pytest.mark.gpu


def _field(dev, width, nhd, nb, M, R, seed, dir_gain=1.0, mma=None):
    """Descriptors, packed weights (the dir network's scaled by dir_gain per layer), f16
    encodings and directions of a field of the pipelines' shapes."""
    from atmonr_amd import _lib

    g = torch.Generator(device=dev).manual_seed(seed)
    lib = _lib.load()
    pdsc, ddsc = _lib.mlp_desc(32, 16, width, 1, False), _lib.mlp_desc(19, nb, width, nhd, False)
    pb, db = ctypes.byref(pdsc), ctypes.byref(ddsc)
    pp = torch.randn(lib.anr_mlp_n_params(pb), device=dev, generator=g) * (2.0 / 32) ** 0.5
    pd = torch.randn(lib.anr_mlp_n_params(db), device=dev, generator=g) * (2.0 / width) ** 0.5
    pd = pd * dir_gain
    enc = (torch.rand(M, 32, device=dev, generator=g) * 2 - 1).half()
    dirs = torch.rand(R, 3, device=dev, generator=g)
    packed = torch.empty(lib.anr_ingp_field_packed_size(pb, db), device=dev, dtype=torch.float16)
    _lib.call("anr_ingp_field_pack", pb, db, _lib.F16 if mma is None else mma, pp.data_ptr(),
              pd.data_ptr(), packed.data_ptr(), _lib.stream(dev))
    return {"keep": (pdsc, ddsc), "pb": pb, "db": db, "pp": pp, "pd": pd, "enc": enc,
            "dirs": dirs, "packed": packed, "g": g}


# ------------------------------------------------------------------ 1. field forward
@pytest.mark.parametrize("width,nhd", [(64, 2), (64, 1), (32, 2), (32, 1)])
@pytest.mark.parametrize("n_per_ray,R,M", [(64, 3, 192),    # the uniform-tile form
                                           (48, 5, 233)])   # general form, partial last tile
def test_field_fwd_h_is_half_of_f32_outputs(dev, width, nhd, n_per_ray, R, M):
    """anr_ingp_field_fwd_h stores exactly .half() (round to nearest even) of what
    anr_ingp_field_fwd stores, zeros of the ReLU and overflow to inf included, and nothing
    past row M. The dir network's weights are scaled so that the colour outputs have a
    spread of about 6e4 (finite in f32): some exceed f16's largest finite value, 65,504."""
    from atmonr_amd import _lib

    f = _field(dev, width, nhd, 4, M, R, seed=21, dir_gain=1e5 ** (1.0 / (nhd + 1)))
    s = _lib.stream(dev)
    sig32 = torch.full((M + 16,), float("nan"), device=dev)
    col32 = torch.full((M + 16, 4), float("nan"), device=dev)
    _lib.call("anr_ingp_field_fwd", f["pb"], f["db"], _lib.F16, f["packed"].data_ptr(),
              f["enc"].data_ptr(), 32, f["dirs"].data_ptr(), n_per_ray, M, sig32.data_ptr(),
              col32.data_ptr(), 4, s)
    sig16 = torch.full((M + 16,), float("nan"), device=dev, dtype=torch.float16)
    col16 = torch.full((M + 16, 4), float("nan"), device=dev, dtype=torch.float16)
    _lib.call("anr_ingp_field_fwd_h", f["pb"], f["db"], _lib.F16, f["packed"].data_ptr(),
              f["enc"].data_ptr(), 32, f["dirs"].data_ptr(), n_per_ray, M, sig16.data_ptr(),
              col16.data_ptr(), 4, s)
    torch.cuda.synchronize(dev)
    assert torch.isfinite(sig32[:M]).all() and torch.isfinite(col32[:M]).all()
    assert torch.equal(sig16[:M], sig32[:M].half())
    assert torch.equal(col16[:M], col32[:M].half())
    assert torch.isnan(sig16[M:]).all() and torch.isnan(col16[M:]).all()
    # both kinds of value occur: a negative pre-activation (stored 0) and an overflow
    assert (col16[:M] == 0).any() and (sig16[:M] == 0).any()
    assert torch.isinf(col16[:M]).any() and (col32[:M] > 65504).any()


@pytest.mark.parametrize("n_per_ray,R,M", [(64, 3, 192), (48, 5, 233)])
def test_field_fwd_h_bf16_is_half_of_f32_outputs(dev, n_per_ray, R, M):
    """The same equality with bf16 MFMA (the pipelines run f16 outputs in reference numerics,
    which are f16; the entry takes both), in the uniform-tile and the general form."""
    from atmonr_amd import _lib

    f = _field(dev, 64, 2, 4, M, R, seed=22, mma=_lib.BF16)
    s = _lib.stream(dev)
    sig32 = torch.full((M + 16,), float("nan"), device=dev)
    col32 = torch.full((M + 16, 4), float("nan"), device=dev)
    sig16, col16 = sig32.half(), col32.half()
    for name, sig, col in (("anr_ingp_field_fwd", sig32, col32),
                           ("anr_ingp_field_fwd_h", sig16, col16)):
        _lib.call(name, f["pb"], f["db"], _lib.BF16, f["packed"].data_ptr(), f["enc"].data_ptr(),
                  32, f["dirs"].data_ptr(), n_per_ray, M, sig.data_ptr(), col.data_ptr(), 4, s)
    torch.cuda.synchronize(dev)
    assert torch.isfinite(sig32[:M]).all() and torch.isfinite(col32[:M]).all()
    assert (col32[:M] > 0).any() and (sig32[:M] > 0).any()
    assert torch.equal(sig16[:M], sig32[:M].half())
    assert torch.equal(col16[:M], col32[:M].half())
    assert torch.isnan(sig16[M:]).all() and torch.isnan(col16[M:]).all()


# ------------------------------------------------------------------ 2. field backward
@pytest.mark.parametrize("ws", [False, True])
@pytest.mark.parametrize("M", [384, 233])   # 6 rays x 64 samples; a partial last tile
def test_field_bwd_rows_h_equals_f32_entry(dev, M, ws):
    """anr_ingp_field_bwd_ref16_rows_h on f16 gradients against anr_ingp_field_bwd_ref16_rows
    on the same values as f32: dL/denc rows and row bits bit for bit, the parameter
    gradients up to the f32 atomic flush order (the bound of
    test_ingp_field_bwd_ref16_rows_equals_f32_rows). dL/dcolor is zero on whole 32-row
    tiles and nonzero on others, so with a workspace both the pos pass and the list pass
    run (the listed-tile count is read back)."""
    from atmonr_amd import _lib

    n_per_ray, nb = 64, 4
    R = -(-M // n_per_ray)
    f = _field(dev, 64, 2, nb, M, R, seed=22)
    lib, s, g = _lib.load(), _lib.stream(dev), f["g"]
    dcol = (torch.randn(M, nb, device=dev, generator=g) * 1e-2).half()
    dsig = (torch.randn(M, device=dev, generator=g) * 1e-3).half()
    n_tiles = -(-M // 32)
    zero_tiles = [t for t in range(n_tiles) if t % 3 != 1]   # colour gradients on tiles 1, 4, 7, 10
    for t in zero_tiles:
        dcol[32 * t:32 * (t + 1)] = 0
    dsig[64:96] = 0                                         # tile 2: no gradient at all
    outs = []
    for half in (False, True):
        dc, dsg = (dcol, dsig) if half else (dcol.float(), dsig.float())
        d_enc = torch.full((M, 32), float("nan"), device=dev, dtype=torch.float16)
        bits = torch.full((n_tiles,), -7, device=dev, dtype=torch.int32)
        g_pos, g_dir = torch.zeros_like(f["pp"]), torch.zeros_like(f["pd"])
        wsb = lib.anr_ingp_field_bwd_ref16_rows_workspace_bytes(M) if ws else 0
        wst = torch.zeros(max(1, wsb), device=dev, dtype=torch.uint8)
        _lib.call("anr_ingp_field_bwd_ref16_rows_h" if half else "anr_ingp_field_bwd_ref16_rows",
                  f["pb"], f["db"], f["packed"].data_ptr(), f["enc"].data_ptr(), 32,
                  f["dirs"].data_ptr(), n_per_ray, M, dsg.data_ptr(), dc.data_ptr(), nb,
                  d_enc.data_ptr(), 32, g_pos.data_ptr(), g_dir.data_ptr(), 128.0,
                  bits.data_ptr(), wst.data_ptr() if ws else None, wsb, s)
        torch.cuda.synchronize(dev)
        listed = int(wst[:4].view(torch.int32).item()) if ws else None
        outs.append((d_enc, bits, g_pos, g_dir, listed))
    (d32, b32, gp32, gd32, n32), (d16, b16, gp16, gd16, n16) = outs
    assert torch.isfinite(d32.float()).all()
    assert torch.equal(d16, d32) and torch.equal(b16, b32)
    assert (d32 != 0).any()
    if ws:  # both passes ran, over the same tiles in both forms
        assert n16 == n32 == n_tiles - len(zero_tiles)
        assert 0 < n16 < n_tiles
    for a_, b_ in ((gp16, gp32), (gd16, gd32)):
        assert b_.abs().max().item() > 0
        assert (a_ - b_).abs().max().item() <= 2e-5 * b_.abs().max().item()


# ------------------------------------------------------------------ 3. composite backward
@pytest.mark.parametrize("surface", [True, False])
@pytest.mark.parametrize("N,C", [(70, 4), (64, 4), (70, 1), (64, 1)])
def test_composite_bwd_f16_io_bit_exact(dev, N, C, surface):
    """f16 inputs and f16 gradient outputs against oracle/ref_f16.py, bit for bit: C = 4
    parks T_k and exp(-sigma delta) as one 4-byte pair per sample in the ray's d_color
    rows, C = 1 keeps the two 2-byte slots; N = 70 has a 6-sample segment tail. Two rays
    have an f16 alpha of exactly 1: counted, their gradients zero, their neighbours exact."""
    from atmonr_amd.graphics_utils import render_with_surface_ref16

    B = 11
    rng = np.random.default_rng(7)
    z = (np.sort(rng.random((B, N)), 1) * 22.7 / 100.0).astype(np.float32)
    sigma = ref_f16.h(rng.random((B, N, 1)) * 0.5)
    color = ref_f16.h(rng.random((B, N, C)))
    cs = ref_f16.h(rng.random((B, C)))
    g = ref_f16.h((rng.random((B, C)) - 0.5) * 2e-3)
    hot = [2, 9]
    sigma[hot, N // 2] = np.float16(6e4)
    t = lambda a: torch.from_numpy(a).to(dev, torch.float16).requires_grad_()  # noqa: E731
    tc, ts, tcs = t(color), t(sigma), (t(cs) if surface else None)
    zr = torch.zeros(1, dtype=torch.int32, device=dev)
    out = render_with_surface_ref16(torch.from_numpy(z).to(dev), tc, ts, tcs, z_scale=100.0,
                                    zero_rays=zr, inputs_f16=True)
    out[0].backward(torch.from_numpy(g).to(dev).half())
    assert tc.grad.dtype == torch.float16 and ts.grad.dtype == torch.float16
    assert int(zr.item()) == len(hot)
    # f16 inputs: the f16 colour / sigma results are the inputs themselves (no copies)
    assert out[-2].data_ptr() == tc.data_ptr() and out[-1].data_ptr() == ts.data_ptr()
    cold = [b for b in range(B) if b not in hot]
    r = ref_f16.render_fwd(z[cold] * np.float32(100.0), color[cold], sigma[cold],
                           cs[cold] if surface else None, acc="cuda")
    gb = ref_f16.render_bwd(r, g[cold], acc="cuda")
    pairs = [(out[0][cold], r["color_map"]), (tc.grad[cold], gb["color"]),
             (ts.grad[cold], gb["sigma"])]
    if surface:
        pairs.append((tcs.grad[cold], gb["cs"]))
    for got, want in pairs:
        a = got.detach().float().cpu().numpy().reshape(want.shape)
        assert np.array_equal(a, want), (np.abs(a - want).max(), int((a != want).sum()))
    assert np.count_nonzero(gb["sigma"]) > 0 and np.count_nonzero(gb["color"]) > 0
    assert not tc.grad[hot].any() and not ts.grad[hot].any()


# ------------------------------------------------------------------ 4. the whole step
_FWD_KEYS = ("color_fine", "color_surf", "color_map_surf", "color_map_atmo", "sigma_fine",
             "color_map_fine", "weights_fine", "z_vals_fine")


def _step(dev, scene, f16_io, hash_field):
    """One eager reference-numerics step from the seeded parameters: forward results, loss,
    every module's gradient, and the dtype the field handed the composite."""
    from atmonr_amd import field
    from atmonr_amd.batch_loader import BatchLoader
    from atmonr_amd.pipelines.instant_ngp import InstantNGPPipeline

    B, N = 8, 64
    mp = pytest.MonkeyPatch()
    try:
        mp.setattr(field, "_REF_F16_IO", f16_io)
        mp.setattr(field, "_HASH_FIELD", hash_field)
        p = InstantNGPPipeline(ge._ingp_config(N), scene, dtype=torch.float16, fused=True, seed=5,
                               numerics="reference")
        p.send_tensors_to(dev)
        p._keep_d_enc = True
        batch = next(iter(BatchLoader(scene, B, seed=1)))
        u = torch.rand(B, N, generator=torch.Generator().manual_seed(2)).to(dev)
        res = p.forward(batch, u=u)
        loss = p.compute_loss(batch, res)
        loss.backward()
        torch.cuda.synchronize(dev)
    finally:
        mp.undo()
    out = {k: res[k].detach().clone() for k in _FWD_KEYS}
    out["loss"] = loss.detach().clone()
    grads = {m: getattr(p, m).params.grad.detach().double().cpu()
             for m in p.module_names if getattr(p, m).params.numel()}
    d_sigma, d_color = p._last_field_grads
    assert p._last_d_enc.dtype == torch.float16   # the diagnostics still see the f16 rows
    return out, grads, (d_sigma.dtype, d_color.dtype), int(p._zero_rays.item())


@pytest.fixture(scope="module")
def scene(dev):
    from atmonr_amd.datasets.synthetic import SyntheticHARP2Dataset

    return SyntheticHARP2Dataset(n_views=8, img_size=16, device=dev, seed=0)


@pytest.fixture(scope="module")
def step_f32_io(dev, scene):
    """The step with f32 interchange (ANR_REF_F16_IO=0: the old entry points), run once."""
    return _step(dev, scene, False, False)


@pytest.mark.parametrize("hash_field", [False, True])
def test_step_same_with_f16_io(dev, scene, step_f32_io, hash_field):
    """The step with the switch on equals the step with it off: forward results and loss bit
    for bit, each module's gradient within the bound test_ingp_oracle_gpu.py holds the
    reference numerics to against the oracle (relative L2 3e-4; the two chains compute the
    same values, only the f32 atomics' order differs). hash_field: the fused hash + field
    forward, whose outputs stay f32 -- the composite then writes its f16 copies and the
    field backward reads f32 gradients, whatever the switch says."""
    out0, grads0, dt0, zr0 = step_f32_io
    out1, grads1, dt1, zr1 = _step(dev, scene, True, hash_field)
    assert dt0 == (torch.float32, torch.float32)
    assert dt1 == ((torch.float32,) * 2 if hash_field else (torch.float16,) * 2)
    assert zr0 == 0 and zr1 == 0
    for k in out0:
        assert out0[k].dtype == out1[k].dtype, k
        assert torch.equal(out0[k], out1[k]), k
    assert out1["color_fine"].dtype == torch.float16 and out1["sigma_fine"].dtype == torch.float16
    assert sorted(grads0) == sorted(grads1)
    assert grads0["pos_encoder"].norm().item() > 0 and grads0["pos_mlp"].norm().item() > 0
    for m, g0 in grads0.items():
        if g0.norm().item() == 0:  # dir_mlp at the seed: the f16 composite underflows dL/dcolor
            assert not grads1[m].any(), m
            continue
        rel = ((grads1[m] - g0).norm() / g0.norm()).item()
        print(f"grad {m}: relative L2 difference {rel:.3e}")
        assert rel <= 3e-4, (m, rel)
