"""The forward-only render on the GPU: InstantNGPPipeline.render / anr_ingp_render against
the existing forward. Reference numerics bit for bit (also with an f16 alpha of exactly 1),
build numerics against an f64 composite within twice the existing forward's own error, the
fallbacks equal to forward, no side effects, the memory a render holds, and render_rays /
render_images; NeRFPipeline.render against its forward. Every Instant-NGP case scales the
hash table until the composite is alive on the existing forward's outputs
(tests/render_checks.py)."""

import copy

import pytest
import torch

import __graft_entry__ as ge
from tests import render_checks as rc

pytestmark = pytest.mark.gpu

KEYS = ("color_map_fine", "color_map_atmo", "color_map_surf", "z_vals_fine")


@pytest.fixture(scope="module")
def scene(dev):
    from atmonr_amd.datasets.synthetic import SyntheticHARP2Dataset

    return SyntheticHARP2Dataset(n_views=8, img_size=16, device=dev, seed=0)


def _config(n, width=64, dir_layers=2, **top):
    cfg = copy.deepcopy(ge._ingp_config(n))
    cfg["instant_ngp"]["network"]["n_neurons"] = width
    cfg["instant_ngp"]["rgb_network"]["n_neurons"] = width
    cfg["instant_ngp"]["rgb_network"]["n_hidden_layers"] = dir_layers
    cfg.update(top)
    return cfg


def _pipe(scene, dev, cfg, **kw):
    from atmonr_amd.pipelines.instant_ngp import InstantNGPPipeline

    p = InstantNGPPipeline(cfg, scene, seed=5, **kw)
    p.send_tensors_to(dev)
    return p


def _batch(scene, dev, B, N):
    from atmonr_amd.batch_loader import BatchLoader

    batch = next(iter(BatchLoader(scene, B, seed=1)))
    u = torch.rand(B, N, generator=torch.Generator().manual_seed(2)).to(dev)
    return batch, u


def _bits(t):
    assert t.dtype == torch.float16
    return t.contiguous().view(torch.int16)


def _same_bits(a, b, what):
    for k in rc.MAPS:
        assert a[k].shape == b[k].shape and a[k].dtype == b[k].dtype == torch.float16, (what, k)
        diff = int((_bits(a[k]) != _bits(b[k])).sum())
        assert diff == 0, f"{what}: {k} differs in {diff} of {a[k].numel()} values"
    assert torch.equal(a["z_vals_fine"], b["z_vals_fine"]), what


# ------------------------------------------------------------------ 1. reference numerics
SMALL = [(5, 64), (40, 128)]
CASES = [(B, N, W, L) for (B, N) in SMALL for W in (32, 64) for L in (1, 2)] + [(3, 1024, 64, 2)]


@pytest.mark.parametrize("B,N,width,dir_layers", CASES)
def test_reference_numerics_bit_for_bit(scene, dev, B, N, width, dir_layers):
    """render equals forward as int16 bit patterns in all three maps, at explicit draws and
    at the bin midpoints, and a second render returns the same bits. (5, 64): one segment and
    a ragged last block; (40, 128): one carry; (3, 1024): the workload's depth."""
    p = _pipe(scene, dev, _config(N, width, dir_layers), numerics="reference")
    assert p.render_kernel_refusal() is None
    batch, u = _batch(scene, dev, B, N)
    # bin midpoints: the sampler's t = 0.5, forward's random=False draws
    half = torch.full((B, N), 0.5, device=dev)

    def alive_at_midpoints(_):
        with torch.no_grad():
            return rc.alive(p.forward(batch, u=half))

    _, fwd = rc.make_alive(p, batch, u, extra=alive_at_midpoints)
    ren = p.render(batch, u=u, fused=True)
    _same_bits(ren, fwd, "explicit draws")
    with torch.no_grad():
        mid = p.forward(batch, u=half)
    ren_mid = p.render(batch, fused=True)
    _same_bits(ren_mid, mid, "midpoints")
    _same_bits(p.render(batch), ren_mid, "second call")
    _same_bits(p.render(batch, u=u), ren, "second call, explicit draws")


def test_reference_numerics_with_bf16_mfma(scene, dev, monkeypatch):
    """anr_ingp_render takes reference numerics with bf16 MFMA, a pair no pipeline asks for
    (reference numerics are tcnn's f16). It keeps the contract of the f16 case: its maps are
    the bits of the two-kernel forward (hash planes, anr_ingp_field_fwd_h, the f16 composite)
    run on the same bf16 weights. (40, 128): one carry, as above. The f16 render of the same
    rays differs, so the bf16 kernels did run."""
    from atmonr_amd import _lib, field

    B, N = 40, 128
    p = _pipe(scene, dev, _config(N), numerics="reference")
    assert p.render_kernel_refusal() is None
    batch, u = _batch(scene, dev, B, N)
    with monkeypatch.context() as m:
        m.setattr(field, "_mma_code", lambda pipe: _lib.BF16)
        _, fwd = rc.make_alive(p, batch, u)
        ren = p.render(batch, u=u, fused=True)
    _same_bits(ren, fwd, "bf16 MFMA")
    ren_f16 = p.render(batch, u=u, fused=True)
    assert any(not torch.equal(ren_f16[k], ren[k]) for k in rc.MAPS)


# ------------------------------------------------------------------ 2. an f16 alpha of 1
def test_alpha_of_exactly_one(scene, dev):
    """Scaled until some sample has sigma * delta > 9 (exp rounds to 0 in f16, alpha to 1, q2
    to 0: the ray's transmittance is exactly 0 from there on): still forward's bits, and
    zero_rays_total, which the backward of such rays moves, is not moved by render."""
    B, N = 40, 128
    # W = 32 with one dir layer: at seed 5 its density is zero on four samples of five, so
    # the rays' optical depths spread far enough for an opaque sample on one ray while
    # another ray still has an f16 transmittance above 0
    p = _pipe(scene, dev, _config(N, 32, 1), numerics="reference")
    batch, u = _batch(scene, dev, B, N)

    def saturated(res):
        z = (res["z_vals_fine"] * (p.scale / 1000)).double()
        mid = torch.cat([z[:, :1] * 0, (z[:, :-1] + z[:, 1:]) / 2, z[:, -1:]], dim=1)
        x = (res["sigma_fine"][..., 0].double() * torch.diff(mid, dim=1)[:, :-1]).max().item()
        return x > 9, f"largest sigma * delta {x:.3g}"

    _, fwd = rc.make_alive(p, batch, u, extra=saturated)
    assert (fwd["color_map_surf"] == 0).all(dim=1).any()  # some ray is opaque
    # a training step on these rays counts them
    loss = p.compute_loss(batch, p.forward(batch, u=u))
    loss.backward()
    before = p.zero_rays_total
    assert before > 0
    ren = p.render(batch, u=u, fused=True)
    _same_bits(ren, fwd, "alpha == 1")
    assert p.zero_rays_total == before


# ------------------------------------------------------------------ 3. build numerics
@pytest.mark.parametrize("mlp_dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("B,N", [(40, 128), (3, 1024)])
def test_build_numerics_against_f64(scene, dev, B, N, mlp_dtype):
    """e = largest distance to the f64 composite of the existing field forward's per-sample
    sigma and colour, over the yardstick's largest magnitude, per map: e_render <=
    max(2 e_forward, 2^-22) and <= 1e-4. render and forward differ only in the order of f32
    sums over N terms (a factor of 2 covers an order change, the floor a forward that lands
    within an ulp); the bar hangs on the existing kernel, not on the one under test. The
    yardstick is render_surface_f64's arithmetic with a colour per sample
    (render_checks.f64_maps: that function takes one colour per ray, where the two are
    checked to agree)."""
    p = _pipe(scene, dev, _config(N), mlp_dtype=mlp_dtype)
    assert p.numerics == "build" and p.render_kernel_refusal() is None
    batch, u = _batch(scene, dev, B, N)
    rc.make_alive(p, batch, u)
    errs = rc.composite_errors(p, batch, u)
    for k, (e_render, e_forward) in errs.items():
        print(f"{k}: e_render {e_render:.3e}  e_forward {e_forward:.3e}")
    for k, (e_render, e_forward) in errs.items():
        assert e_render <= max(2 * e_forward, 2.0 ** -22), (k, e_render, e_forward)
        assert e_render <= 1e-4, (k, e_render)
    ren = p.render(batch, u=u)
    assert all(ren[k].dtype == torch.float32 for k in rc.MAPS)


# ------------------------------------------------------------------ 4. fallbacks
FALLBACKS = {
    "n96": dict(cfg=dict(n=96)),
    "include_height": dict(cfg=dict(n=64, include_height=True, point_preprocessor=None)),
    "multi_band": dict(cfg=dict(n=64, multi_band_extinction=True)),
    "f32_modules": dict(cfg=dict(n=64), kw=dict(dtype=torch.float32)),
}


@pytest.mark.parametrize("name", sorted(FALLBACKS))
def test_fallbacks_equal_forward(scene, dev, name):
    from atmonr_amd._lib import ANRError

    spec = FALLBACKS[name]
    cfg = dict(spec["cfg"])
    N = cfg.pop("n")
    p = _pipe(scene, dev, _config(N, **cfg), **spec.get("kw", {}))
    assert p.render_kernel_refusal() is not None
    B = 24
    batch, u = _batch(scene, dev, B, N)
    _, fwd = rc.make_alive(p, batch, u)
    ren = p.render(batch, u=u)
    assert sorted(ren) == sorted(KEYS)
    for k in KEYS:
        assert ren[k].dtype == fwd[k].dtype and torch.equal(ren[k], fwd[k]), (name, k)
    with pytest.raises(ANRError, match="fused=True"):
        p.render(batch, u=u, fused=True)


@pytest.mark.parametrize("numerics", ["build", "reference"])
def test_fused_false_is_forward(scene, dev, numerics):
    B, N = 24, 64
    p = _pipe(scene, dev, _config(N), numerics=numerics)
    assert p.render_kernel_refusal() is None
    batch, u = _batch(scene, dev, B, N)
    _, fwd = rc.make_alive(p, batch, u)
    ren = p.render(batch, u=u, fused=False)
    assert sorted(ren) == sorted(KEYS)
    for k in KEYS:
        assert ren[k].dtype == fwd[k].dtype and torch.equal(ren[k], fwd[k]), k
    with torch.no_grad():
        mid = p.forward(batch, u=torch.full((B, N), 0.5, device=dev))
    ren = p.render(batch, fused=False)
    for k in KEYS:
        assert torch.equal(ren[k], mid[k]), k


# ------------------------------------------------------------------ 5. no side effects
def _step(p, batch, u):
    for m in p.modules():
        m.params.grad = None
    loss = p.compute_loss(batch, p.forward(batch, u=u))
    loss.backward()
    torch.cuda.synchronize()
    return loss.detach().clone(), {n: getattr(p, n).params.grad.detach().clone()
                                   for n in p.module_names if getattr(p, n).params.numel()}


@pytest.mark.parametrize("numerics", ["build", "reference"])
@pytest.mark.parametrize("fused", [True, False])
def test_render_has_no_side_effects(scene, dev, numerics, fused):
    """One ray of 64 samples: the step's parameter gradients are sums of f32 atomics, and
    only where no two wavefronts add into one address is their order, and so every bit of
    the sum, the same from run to run -- which a bit-for-bit comparison of two steps needs
    whether or not a render ran in between."""
    B, N = 1, 64
    p = _pipe(scene, dev, _config(N), numerics=numerics)
    batch, u = _batch(scene, dev, B, N)
    rc.make_alive(p, batch, u)
    loss0, grads0 = _step(p, batch, u)  # the step without a render
    held = {n: getattr(p, n).params.grad for n in grads0}
    zr, training = p.zero_rays_total, p.training
    for inside in (False, True):
        with torch.set_grad_enabled(not inside):
            ren = p.render(batch, u=u, fused=fused)
        assert all(not ren[k].requires_grad and ren[k].grad_fn is None for k in KEYS)
        assert torch.is_grad_enabled()
    assert p.training is training and p.zero_rays_total == zr and p.occupancy is None
    for n, g in grads0.items():  # every params.grad is the same tensor with the same bits
        assert getattr(p, n).params.grad is held[n] and torch.equal(held[n], g), n
    loss1, grads1 = _step(p, batch, u)  # the same step after the renders
    assert torch.equal(loss1, loss0)
    for n in grads0:
        diff = int((grads1[n] != grads0[n]).sum())
        assert diff == 0, f"{n}: {diff} of {grads0[n].numel()} gradient values differ"
    p.eval()
    p.render(batch, u=u, fused=fused)
    assert p.training is False


# ------------------------------------------------------------------ 6. memory
@pytest.mark.parametrize("numerics", ["build", "reference"])
def test_memory_of_a_render(scene, dev, numerics):
    """At (256, 1024) a fused render's peak rises by less than 32 B per sample (its own
    per-sample tensors are coords and z: 16 B), forward's path by more than 64 B (the
    level-quad planes alone)."""
    B, N = 256, 1024
    p = _pipe(scene, dev, _config(N), numerics=numerics)
    batch, u = _batch(scene, dev, B, N)

    def rise(fused):
        p.render(batch, u=u, fused=fused)  # the f16 table copy and the bins exist afterwards
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats(dev)
        base = torch.cuda.memory_allocated(dev)
        out = p.render(batch, u=u, fused=fused)
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated(dev)
        del out
        return (peak - base) / (B * N)

    r_fused, r_forward = rise(True), rise(False)
    print(f"bytes per sample: fused {r_fused:.1f}, forward {r_forward:.1f}")
    assert r_fused < 32
    assert r_forward > 64


# ------------------------------------------------------------------ 7. render_rays / _images
@pytest.mark.parametrize("numerics", ["build", "reference"])
def test_render_rays_and_images(scene, dev, numerics):
    from atmonr_amd.render import render_images, render_rays

    N = 64
    p = _pipe(scene, dev, _config(N), numerics=numerics)
    batch, u = _batch(scene, dev, 40, N)
    rc.make_alive(p, batch, u)
    idx = batch["idx"]
    one = p.render(scene.__getbatch__(idx))
    cut = render_rays(p, scene, idx=idx, batch_size=7)
    for k in rc.MAPS:  # rays are independent: 40 rays in batches of 7 equal one call
        assert cut[k].shape == (40, 4) and torch.equal(cut[k], one[k]), k
    # the whole scene as images, against forward's maps scattered the same way
    pred, metrics = render_images(p, scene, batch_size=1000)
    n = len(scene)
    pix = torch.empty(n, device=dev)
    with torch.no_grad():
        for s in range(0, n, 1000):
            b = scene.__getbatch__(torch.arange(s, min(n, s + 1000), device=dev))
            cm = p.forward(b, u=torch.full((b["origin"].shape[0], N), 0.5, device=dev))
            pix[s:s + 1000] = torch.take_along_dim(cm["color_map_fine"], b["irgb_idx"][:, None],
                                                   dim=1)[:, 0]
    want = scene.get_image_metrics(scene.scatter_image(pix), scene.target_image())
    assert pred.shape == scene.target_image().shape

    def same(got, tol):
        assert sorted(got) == sorted(want)
        for k in want:
            a, b = torch.as_tensor(got[k]).double(), torch.as_tensor(want[k]).double()
            assert torch.allclose(a, b, rtol=tol, atol=tol, equal_nan=True), (k, a, b)

    # forward's own path: forward's pixels and metrics exactly
    pred_f, metrics_f = render_images(p, scene, batch_size=1000, fused=False)
    assert torch.equal(pred_f, scene.scatter_image(pix))
    same(metrics_f, 0.0)
    if numerics == "reference":  # the kernel's maps are forward's bits
        assert torch.equal(pred, pred_f)
        same(metrics, 0.0)
    else:  # forward's maps to the rounding of an f32 sum: the composite bar, 1e-4
        assert (pred - pred_f).abs().max() <= 1e-4 * pred_f.abs().max()
        same(metrics, 1e-4)


# ------------------------------------------------------------------ NeRFPipeline.render
def test_nerf_render_is_forward_without_grad(dev):
    from atmonr_amd._lib import ANRError
    from atmonr_amd.batch_loader import BatchLoader
    from atmonr_amd.datasets.synthetic import SyntheticHARP2Dataset
    from atmonr_amd.pipelines.nerf import NeRFPipeline

    ds = SyntheticHARP2Dataset(n_views=4, img_size=8, device=dev, seed=0)
    cfg = {"type": "NeRF", "include_height": False, "point_preprocessor": "horizontal",
           "num_bands": 4, "ray_origin_height": 20000, "sampler": {"N_c": 16, "N_f": 24},
           "encoder": {"L_x": [14, 14, 10], "L_d": 4}, "mlp_hidden_dim": 32}
    p = NeRFPipeline(cfg, ds)
    p.send_tensors_to(dev)
    p.eval()  # no density noise: a render is deterministic
    B = 9
    batch = next(iter(BatchLoader(ds, B, seed=1)))
    u_c = torch.full((B, 16), 0.5, device=dev)
    u_f = ((torch.arange(24, device=dev) + 0.5) / 24)[None].repeat(B, 1)
    with torch.no_grad():
        fwd = p.forward(batch, u_coarse=u_c, u_fine=u_f)
    ren = p.render(batch)
    assert sorted(ren) == ["color_map_coarse", "color_map_fine", "z_vals_fine"]
    for k, v in ren.items():
        assert not v.requires_grad and torch.equal(v, fwd[k]), k
    again = p.render(batch, u=(u_c, u_f), fused=False)
    assert all(torch.equal(again[k], ren[k]) for k in ren)
    assert p.training is False
    with pytest.raises(ANRError, match="fused=True"):
        p.render(batch, fused=True)
