"""The 4-D hash-grid kernels (include_height) against the oracle.

The oracle (oracle/ref_tcnn.py) is dimension-generic apart from its prime table, whose
fourth entry the tests set at run time. f32 tables, tolerances as the 3-D test of
tests/test_kernels_gpu.py: forward rel 1e-5, backward rel 1e-5 / atol 1e-5. The fourth
coordinate, the normalised height, is not confined to [0, 1]: it spans [-20, 20] here, so
dense levels wrap modulo their size and hashed levels hash the wrapped (negative) cells."""

import ctypes

import numpy as np
import pytest
import torch

from oracle import ref_tcnn

pytestmark = pytest.mark.gpu

SMALL = (4, 4, 4, 1.5, 10)       # one dense level, one hashed with res^3 <= T, two early-stop
CONFIG3 = (4, 16, 16, 1.3819, 19)


@pytest.fixture(autouse=True)
def _four_primes(monkeypatch):
    monkeypatch.setattr(ref_tcnn, "PRIMES",
                        np.array([1, 2654435761, 805459861, 3674653429], dtype=np.uint32))


def close(a, b, rel, atol=1e-7):
    a = torch.as_tensor(a).double().cpu()
    b = torch.as_tensor(b).double().cpu()
    assert a.shape == b.shape, (a.shape, b.shape)
    err = (a - b).abs().max().item()
    tol = rel * b.abs().max().item() + atol
    print(f"max err {err:.3e} tol {tol:.3e}")
    assert err <= tol, f"max err {err:.3e} > tol {tol:.3e}"


def _points(M, coherent, seed=0, n_per_ray=256):
    """Random points, or ray-like ones (consecutive samples on straight lines, so that the
    walkers' cell-reuse path runs); column 3 spans [-20, 20] either way."""
    gen = torch.Generator().manual_seed(seed)
    if coherent:
        R = -(-M // n_per_ray)
        o = torch.rand(R, 1, 4, generator=gen)
        d = (torch.rand(R, 1, 4, generator=gen) - 0.5) * 0.3
        o[..., 3] = o[..., 3] * 40 - 20
        d[..., 3] = d[..., 3] * 4
        t = torch.linspace(0, 1, n_per_ray)[None, :, None]
        x = o + d * t
        x[..., :3] = x[..., :3].clamp(0, 1)
        x = x.reshape(-1, 4)[:M]
    else:
        x = torch.rand(M, 4, generator=gen)
        x[:, 3] = x[:, 3] * 40 - 20
        x[0, 0] = 1.0  # the far face: a corner at res
    return x.contiguous()


def _fwd(d, x, table, out_dtype=torch.float32):
    from atmonr_amd import _lib

    out = torch.empty(x.shape[0], d.n_levels * 2, device=x.device, dtype=out_dtype)
    _lib.call("anr_hashgrid_fwd", ctypes.byref(d), x.data_ptr(), x.stride(0), x.shape[0],
              table.data_ptr(), _lib.dtype_code(table.dtype), out.data_ptr(),
              _lib.dtype_code(out_dtype), out.stride(0), _lib.stream(x.device))
    return out


def _bwd(d, x, dout, entry="anr_hashgrid_bwd", *extra):
    from atmonr_amd import _lib

    dtab = torch.zeros(d.n_params, device=x.device)
    _lib.call(entry, ctypes.byref(d), x.data_ptr(), x.stride(0), x.shape[0], dout.data_ptr(),
              _lib.dtype_code(dout.dtype), dout.stride(0), dtab.data_ptr(), *extra,
              _lib.stream(x.device))
    return dtab


@pytest.mark.parametrize("cfg,M,coherent", [(SMALL, 777, False), (SMALL, 4096, True),
                                            (CONFIG3, 5000, False), (CONFIG3, 8192, True)])
def test_hashgrid4d_fwd_bwd_f32(dev, cfg, M, coherent):
    from atmonr_amd import _lib

    d = _lib.hashgrid_desc(4, cfg[1], 2, cfg[2], cfg[3], cfg[4], allow_4d=True)
    gen = torch.Generator().manual_seed(1)
    table = torch.rand(d.n_params, generator=gen) * 2 - 1
    x = _points(M, coherent)
    if not coherent:
        assert x[0, 0] == 1.0 and x[:, 3].min() < -15 and x[:, 3].max() > 15
    xd = x.to(dev)
    out = _fwd(d, xd, table.to(dev))
    close(out, ref_tcnn.hashgrid_fwd(x.numpy(), table.numpy(), cfg), rel=1e-5)
    dout = torch.randn(M, cfg[1] * 2, generator=gen)
    dtab = _bwd(d, xd, dout.to(dev))
    gref = ref_tcnn.hashgrid_bwd(x.numpy(), dout.numpy(), cfg, d.n_params // 2)
    close(dtab, gref, rel=1e-5, atol=1e-5)


@pytest.mark.parametrize("n_features", [1, 4, 8])
def test_hashgrid4d_other_feature_counts(dev, n_features):
    from atmonr_amd import _lib

    cfg, M = SMALL, 777
    d = _lib.hashgrid_desc(4, cfg[1], n_features, cfg[2], cfg[3], cfg[4], allow_4d=True)
    gen = torch.Generator().manual_seed(2)
    table = torch.rand(d.n_params, generator=gen) * 2 - 1
    x = _points(M, False)
    xd, td = x.to(dev), table.to(dev)
    s = _lib.stream(dev)
    out = torch.empty(M, cfg[1] * n_features, device=dev)
    _lib.call("anr_hashgrid_fwd", ctypes.byref(d), xd.data_ptr(), 4, M, td.data_ptr(), _lib.F32,
              out.data_ptr(), _lib.F32, out.stride(0), s)
    close(out, ref_tcnn.hashgrid_fwd(x.numpy(), table.numpy(), cfg, n_features), rel=1e-5)
    dout = torch.randn(M, cfg[1] * n_features, generator=gen)
    dtab = _bwd(d, xd, dout.to(dev))
    gref = ref_tcnn.hashgrid_bwd(x.numpy(), dout.numpy(), cfg, d.n_params // n_features,
                                 n_features)
    close(dtab, gref, rel=1e-5, atol=1e-5)


@pytest.mark.parametrize("cfg", [SMALL, CONFIG3])
@pytest.mark.parametrize("M", [8192, 1000])
@pytest.mark.parametrize("tdt", ["f16", "f32"])
def test_hashgrid4d_planes_equal_rows_bit_for_bit(dev, cfg, M, tdt):
    """anr_hashgrid_fwd_planes (one lane per sample, 16 corner gathers per level) against
    the row-layout forward in f16, as the 3-D check of test_hashgrid_fwd_v6_outside_grid_
    and_strides: equal bits, a partial last quad zero-filled, nothing written past row M."""
    from atmonr_amd import _lib

    L = cfg[1]
    d = _lib.hashgrid_desc(4, L, 2, cfg[2], cfg[3], cfg[4], allow_4d=True)
    gen = torch.Generator(device=dev).manual_seed(11)
    x = _points(M, True, seed=3, n_per_ray=97).to(dev)
    x[::7, :3] = x[::7, :3].round()  # exact faces too
    dt = torch.float16 if tdt == "f16" else torch.float32
    table = ((torch.rand(d.n_params, device=dev, generator=gen) * 2 - 1) * 1e-2).to(dt)
    rows = _fwd(d, x, table, dt)
    plane = 8 * M + 16
    nq = -(-L // 4)
    pl = torch.full((nq * plane + 8,), -9.0, device=dev, dtype=torch.float16)
    _lib.call("anr_hashgrid_fwd_planes", ctypes.byref(d), x.data_ptr(), 4, M, table.data_ptr(),
              _lib.dtype_code(dt), pl.data_ptr(), plane, _lib.stream(dev))
    got = torch.cat([pl[q * plane:q * plane + 8 * M].view(M, 8) for q in range(nq)], 1)
    assert torch.equal(got[:, :2 * L], rows.half())
    assert torch.all(got[:, 2 * L:] == 0)
    for q in range(nq):
        assert torch.all(pl[q * plane + 8 * M:(q + 1) * plane] == -9)


def test_hashgrid4d_adjoint_identity(dev):
    """<g, fwd(t)> = <bwd(g), t> over 64 rays x 1024 samples of the config-3 grid: a missed
    or doubled corner flush at a chunk end would break it by ~1e-3 of the scale."""
    from atmonr_amd import _lib

    B, N = 64, 1024
    d = _lib.hashgrid_desc(4, 16, 2, 16, 1.3819, 19, allow_4d=True)
    gen = torch.Generator(device=dev).manual_seed(7)
    x = _points(B * N, True, seed=5, n_per_ray=N).to(dev)
    table = torch.rand(d.n_params, device=dev, generator=gen) * 2 - 1
    out = _fwd(d, x, table)
    g = torch.randn(B * N, 32, device=dev, generator=gen)
    dtab = _bwd(d, x, g)
    lhs = torch.dot(g.flatten().double(), out.flatten().double()).item()
    rhs = torch.dot(dtab.double(), table.double()).item()
    scale = torch.dot(g.flatten().double().abs(), out.flatten().double().abs()).item()
    print(f"lhs {lhs:.9e} rhs {rhs:.9e} scale {scale:.3e}")
    assert abs(lhs - rhs) <= 1e-5 * scale, (lhs, rhs, scale)


@pytest.mark.parametrize("gdt", [torch.float32, torch.float16])
def test_hashgrid4d_bwd_rows_falls_back_to_the_plain_backward(dev, gdt):
    """anr_hashgrid_bwd_rows outside its 3-D walker: the rows whose bit is clear (two in
    three here) are zeroed in place and the plain backward runs; the tile form ignores its
    flags the same way, and the request counter refuses the shape."""
    from atmonr_amd import _lib

    M = 64 * 96
    d = _lib.hashgrid_desc(4, 16, 2, 16, 1.3819, 19, allow_4d=True)
    gen = torch.Generator(device=dev).manual_seed(9)
    x = _points(M, True, seed=6, n_per_ray=96).to(dev)
    g = (torch.randn(M, 32, device=dev, generator=gen) * 1e-2).to(gdt)
    keep = (torch.arange(M, device=dev) % 3) == 0
    w = torch.zeros(-(-M // 32) * 32, device=dev, dtype=torch.int64)
    w[:M] = keep
    bits = (w.view(-1, 32) << torch.arange(32, device=dev)).sum(1)
    row_nz = torch.where(bits >= 2 ** 31, bits - 2 ** 32, bits).to(torch.int32)
    zeroed = torch.where(keep[:, None], g, torch.zeros_like(g))
    want = _bwd(d, x, zeroed)
    g_in = g.clone()
    got = _bwd(d, x, g_in, "anr_hashgrid_bwd_rows", row_nz.data_ptr())
    assert torch.equal(g_in, zeroed)  # the clear rows were zeroed in place
    assert (got - want).abs().max().item() <= 1e-5 * want.abs().max().item()
    tiles = torch.ones(-(-M // 32), device=dev, dtype=torch.uint8)
    got = _bwd(d, x, zeroed, "anr_hashgrid_bwd_tiles", tiles.data_ptr())
    assert (got - want).abs().max().item() <= 1e-5 * want.abs().max().item()
    count = torch.zeros(1, device=dev, dtype=torch.int64)
    rc = _lib.load().anr_hashgrid_bwd_count_requests(
        ctypes.byref(d), x.data_ptr(), 4, M, zeroed.data_ptr(), _lib.dtype_code(gdt), 32,
        want.data_ptr(), count.data_ptr(), _lib.stream(dev))
    assert rc == -3  # ANR_E_UNSUPPORTED


def test_encoding_4d_standalone_forward_and_table_gradient(dev):
    from atmonr_amd.tcnn import Encoding

    cfg = {"otype": "HashGrid", "n_levels": 4, "n_features_per_level": 2,
           "log2_hashmap_size": 10, "base_resolution": 4, "per_level_scale": 1.5}
    enc = Encoding(4, cfg, dtype=torch.float32).to(dev)
    with torch.no_grad():
        enc.params.copy_(torch.rand(enc.params.shape, generator=torch.Generator().manual_seed(3))
                         * 2 - 1)
    x = _points(777, False, seed=4).to(dev)
    out = enc(x)
    assert out.shape == (777, 8)
    d = enc.hash_grids[0].desc
    direct = _fwd(d, x, enc.params.detach())
    assert torch.equal(out.detach().float(), direct)
    g = torch.randn(777, 8, device=dev, generator=torch.Generator(device=dev).manual_seed(5))
    out.backward(g.to(out.dtype))
    want = _bwd(d, x, g)
    assert (enc.params.grad - want).abs().max().item() <= 1e-5 * want.abs().max().item()
