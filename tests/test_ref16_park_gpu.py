"""The parked pair of the reference-numerics composite (csrc/ref16.hip):
anr_composite_ref16_fwd_park leaves T_i, exp(-sigma_i delta_i), the surface product and the
alpha-is-1 flag for anr_composite_ref16_bwd_parked, which then has no replay of the forward.

Bar: BIT-EXACT. The parked forward's outputs and the parked backward's gradients equal the
restatement (oracle/ref_f16.py), the park decodes to the oracle's own T, e and pr, and the
parked gradients equal those of the replay entry point (anr_composite_ref16_bwd) called on
the same inputs. Inputs as tests/test_ref16_gpu.py's _case (seed 0).

Shapes (B, N, smax, C): N on and around the 64-sample segment and the 8-sample LDS vector
(1, 7, 64, 65, 72, 129), ray counts that leave a wave part-filled and one that spans many
blocks, every band-sum lane layout (C = 1, 3, 4, 8), and the settled bench state where
dL/dcolor is all zero (smax = 2e-4)."""

import functools

import numpy as np
import pytest
import torch

from oracle import ref_f16

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 1.0, 4), (17, 1, 0.05, 4), (15, 7, 0.05, 4), (1, 65, 0.2, 4),
          (33, 64, 2.0, 4), (17, 65, 1.0, 3), (19, 129, 0.5, 1), (18, 96, 0.5, 8),
          (37, 200, 0.05, 4), (130, 72, 0.5, 4), (35, 1024, 0.5, 4), (16, 1024, 2e-4, 4)]
ZS = 100.0


def _case(B, N, smax, zmax=22.7, C=4, seed=0):
    rng = np.random.default_rng(seed)
    z = (np.sort(rng.random((B, N)), 1) * zmax / 100.0).astype(np.float32)  # x z_scale 100
    sigma = ref_f16.h(rng.random((B, N, 1)) * smax)
    color = ref_f16.h(rng.random((B, N, C)))
    cs = ref_f16.h(rng.random((B, C)))
    g = ref_f16.h((rng.random((B, C)) - 0.5) * 2e-3)
    return z, sigma, color, cs, g


@functools.lru_cache(maxsize=None)
def _reference(shape, surface):
    """The inputs and the oracle's forward and backward for one shape: computed once,
    shared by the dtype cases, never modified."""
    B, N, smax, C = shape
    z, sigma, color, cs, g = _case(B, N, smax, C=C)
    r = ref_f16.render_fwd(z * np.float32(ZS), color, sigma, cs if surface else None, acc="cuda")
    gb = ref_f16.render_bwd(r, g, acc="cuda")
    # the surface product is formed (and parked) with or without a surface colour
    pr = r["pr"] if surface else ref_f16.render_fwd(z * np.float32(ZS), color, sigma, cs,
                                                    acc="cuda")["pr"]
    return (z, sigma, color, cs, g), r, gb, pr


def _bits(a):
    """f16 values held in an f32 array -> their f16 bit patterns."""
    return np.ascontiguousarray(a, dtype=np.float32).astype(np.float16).view(np.uint16)


def _eq(got, want):
    a = got.detach().float().cpu().numpy().reshape(want.shape)
    assert np.array_equal(a, want), (np.abs(a - want).max(), int((a != want).sum()))


class _Run:
    """One shape on the GPU through the entry points themselves (_lib.call)."""

    def __init__(self, dev, inputs, in_dtype, surface, out_dtype=None):
        z, sigma, color, cs, g = inputs
        self.dev, self.dt, self.od = dev, in_dtype, out_dtype or in_dtype
        self.B, self.N, self.C = color.shape
        self.z = torch.from_numpy(z).to(dev)
        self.color = torch.from_numpy(color).to(dev, in_dtype)
        self.sigma = torch.from_numpy(sigma).to(dev, in_dtype)
        self.cs = torch.from_numpy(cs).to(dev, in_dtype) if surface else None
        self.g = torch.from_numpy(g).to(dev).half()

    def forward(self, alpha=True):
        from atmonr_amd import _lib
        from atmonr_amd._lib import dtype_code, ptr

        B, N, C, dev = self.B, self.N, self.C, self.dev
        e = lambda *s: torch.full(s, float("nan"), device=dev, dtype=torch.float16)  # noqa: E731
        self.cm, self.atmo, self.w = e(B, C), e(B, C), e(B, N)
        self.surf = e(B, C) if self.cs is not None else None
        self.alpha = e(B, N) if alpha else None
        self.park = torch.full((B, N), -1, device=dev, dtype=torch.int32)
        self.ray_park = torch.full((B,), -1, device=dev, dtype=torch.int32)
        _lib.call("anr_composite_ref16_fwd_park", ptr(self.z), ZS, ptr(self.color),
                  ptr(self.sigma), ptr(self.cs), dtype_code(self.dt), B, N, C, ptr(self.cm),
                  ptr(self.atmo), ptr(self.surf), ptr(self.w), ptr(self.alpha), None, None,
                  ptr(self.park), ptr(self.ray_park), _lib.stream(dev))

    def backward(self, parked):
        from atmonr_amd import _lib
        from atmonr_amd._lib import dtype_code, ptr

        B, N, C, dev = self.B, self.N, self.C, self.dev
        e = lambda *s: torch.full(s, float("nan"), device=dev, dtype=self.od)  # noqa: E731
        d_color, d_sigma = e(B, N, C), e(B, N, 1)
        d_cs = e(B, C) if self.cs is not None else None
        zr = torch.zeros(1, dtype=torch.int32, device=dev)
        args = (ptr(self.z), ZS, ptr(self.color), None if parked else ptr(self.sigma),
                ptr(self.cs), dtype_code(self.dt), B, N, C, ptr(self.g), ptr(d_color),
                ptr(d_sigma), ptr(d_cs), dtype_code(self.od), ptr(zr))
        if parked:
            _lib.call("anr_composite_ref16_bwd_parked", *args, ptr(self.park),
                      ptr(self.ray_park), _lib.stream(dev))
        else:
            _lib.call("anr_composite_ref16_bwd", *args, _lib.stream(dev))
        return d_color, d_sigma, d_cs, int(zr.item())

    def park_fields(self):
        pk = self.park.cpu().numpy().view(np.uint32)
        rp = self.ray_park.cpu().numpy().view(np.uint32)
        return ((pk & 0xFFFF).astype(np.uint16), (pk >> 16).astype(np.uint16),
                (rp & 0xFFFF).astype(np.uint16), rp >> 16)


@pytest.fixture
def rays_per_wave():
    """Set the composite kernels' rays per wavefront for one test, restore the default."""
    from atmonr_amd import _lib

    yield lambda r: _lib.call("anr_composite_ref16_set_rays", r)
    _lib.call("anr_composite_ref16_set_rays", 0)


def _check_parked(dev, shape, surface, in_dtype, out_dtype=None):
    inputs, r, gb, pr = _reference(shape, surface)
    B, N = shape[:2]
    run = _Run(dev, inputs, in_dtype, surface, out_dtype)
    run.forward()
    # forward bit-exact
    _eq(run.cm, r["color_map"])
    _eq(run.w, r["w"])
    _eq(run.alpha, r["alpha"])
    _eq(run.atmo, r["atmo"])
    if surface:
        _eq(run.surf, r["surf"])
    # park contents
    T, e, prb, flag = run.park_fields()
    assert np.array_equal(T, _bits(r["T"]).reshape(B, N))
    assert np.array_equal(e, _bits(r["e"]).reshape(B, N))
    assert np.array_equal(prb, _bits(pr).reshape(B))
    assert not flag.any()
    # parked backward: the oracle's gradients, and the replay entry point's
    gc, gs, gcs, zr = run.backward(parked=True)
    assert zr == 0
    _eq(gc, gb["color"])
    _eq(gs, gb["sigma"])
    if surface:
        _eq(gcs, gb["cs"])
    rc, rs, rcs, rzr = run.backward(parked=False)
    assert rzr == 0
    assert torch.equal(gc, rc) and torch.equal(gs, rs)
    if surface:
        assert torch.equal(gcs, rcs)
    assert np.count_nonzero(gb["sigma"]) > 0


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(str(v) for v in s))
@pytest.mark.parametrize("surface", [True, False], ids=["surf", "nosurf"])
@pytest.mark.parametrize("in_dtype", [torch.float16, torch.float32], ids=["f16", "f32"])
def test_parked_pair_bit_exact(dev, shape, surface, in_dtype):
    _check_parked(dev, shape, surface, in_dtype)


@pytest.mark.parametrize("in_dtype,out_dtype", [(torch.float16, torch.float32),
                                                (torch.float32, torch.float16)])
def test_parked_backward_mixed_dtypes(dev, in_dtype, out_dtype):
    """The two in / out dtype combinations the autograd function does not form."""
    _check_parked(dev, (37, 200, 0.05, 4), True, in_dtype, out_dtype)


@pytest.mark.parametrize("R", [2, 4, 8])
@pytest.mark.parametrize("shape", [(37, 200, 0.05, 4), (18, 96, 0.5, 8), (17, 65, 1.0, 3)],
                         ids=lambda s: "x".join(str(v) for v in s))
def test_parked_pair_rays_per_wave(dev, rays_per_wave, shape, R):
    """Several rays per wavefront (halved while R * C > 64), last wave part-filled."""
    rays_per_wave(R)
    _check_parked(dev, shape, True, torch.float16)


def test_parked_pair_default_rule_at_large_ray_counts(dev):
    """From 8,192 rays up the default rule runs 2 rays per wavefront: many blocks, the last
    wave part-filled."""
    _check_parked(dev, (8193, 65, 0.5, 4), True, torch.float16)


@pytest.mark.parametrize("R", [0, 2])
def test_parked_zero_rays_beside_normal_rays(dev, rays_per_wave, R):
    """Rays whose alpha rounds to 1 share wavefronts with ordinary rays: flagged in
    ray_park, counted once per launch, zero gradients; their neighbours bit-exact."""
    rays_per_wave(R)
    B, N = 19, 96
    z, sigma, color, cs, g = _case(B, N, 1e-2)
    hot = [1, 6, 7, 16]
    sigma[hot, 40] = np.float16(6e4)
    run = _Run(dev, (z, sigma, color, cs, g), torch.float16, True)
    run.forward()
    flag = run.park_fields()[3]
    assert np.flatnonzero(flag).tolist() == hot and set(flag.tolist()) <= {0, 1}
    gc, gs, gcs, zr = run.backward(parked=True)
    assert zr == len(hot)
    cold = [b for b in range(B) if b not in hot]
    r = ref_f16.render_fwd(z[cold] * np.float32(ZS), color[cold], sigma[cold], cs[cold],
                           acc="cuda")
    gb = ref_f16.render_bwd(r, g[cold], acc="cuda")
    _eq(run.cm[cold], r["color_map"])
    _eq(gc[cold], gb["color"])
    _eq(gs[cold], gb["sigma"])
    _eq(gcs[cold], gb["cs"])
    assert not gc[hot].any() and not gs[hot].any()


def test_no_park_without_grad(dev):
    """An inference forward returns the same outputs and allocates no park; with a gradient
    to flow the autograd function parks; need_alpha=False drops only alpha."""
    from atmonr_amd.graphics_utils import render_with_surface_ref16

    shape = (130, 72, 0.5, 4)
    (z, sigma, color, cs, g), r, gb, _ = _reference(shape, True)
    B, N, _, C = shape
    tz = torch.from_numpy(z).to(dev)
    tc = torch.from_numpy(color).to(dev).half().requires_grad_()
    ts = torch.from_numpy(sigma).to(dev).half().requires_grad_()
    tcs = torch.from_numpy(cs).to(dev).half().requires_grad_()
    zr = torch.zeros(1, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(dev)
    before = torch.cuda.memory_allocated(dev)
    with torch.no_grad():
        out = render_with_surface_ref16(tz, tc, ts, tcs, z_scale=ZS, zero_rays=zr)
    peak = torch.cuda.max_memory_allocated(dev) - before
    assert out[0].grad_fn is None
    # the five outputs, each rounded up to the allocator's 512-byte block: no room for a park
    outputs = sum(-(-o.numel() * o.element_size() // 512) * 512 for o in out)
    assert peak <= outputs
    for got, want in zip(out, (r["color_map"], r["alpha"], r["w"], r["atmo"], r["surf"])):
        _eq(got, want)
    # a gradient can flow: parked, and the same gradients
    out_g = render_with_surface_ref16(tz, tc, ts, tcs, z_scale=ZS, zero_rays=zr)
    assert out_g[0].grad_fn.parked
    for a, b in zip(out, out_g):
        assert torch.equal(a, b)
    out_g[0].backward(torch.from_numpy(g).to(dev).half())
    _eq(tc.grad, gb["color"])
    _eq(ts.grad, gb["sigma"])
    _eq(tcs.grad, gb["cs"])
    # grad mode on, but nothing requires a gradient: no park either
    out_d = render_with_surface_ref16(tz, tc.detach(), ts.detach(), tcs.detach(), z_scale=ZS,
                                      zero_rays=zr)
    assert out_d[0].grad_fn is None
    # need_alpha=False
    with torch.no_grad():
        out_n = render_with_surface_ref16(tz, tc, ts, tcs, z_scale=ZS, zero_rays=zr,
                                          need_alpha=False)
    assert out_n[1] is None and len(out_n) == len(out)
    for k in (0, 2, 3, 4):
        assert torch.equal(out_n[k], out[k])
    assert int(zr.item()) == 0
