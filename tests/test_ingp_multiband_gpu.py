"""InstantNGPPipeline with ``multi_band_extinction: true`` against the oracle, through the
fused path (the fused field kernels with S = num_bands density outputs) and the unfused
op-by-op path.

The oracle is oracle/ref_ingp.RefInstantNGP with the forward of instant_ngp.py:137-206
with the switch on: sigma = relu(pos_out[:, :S]), the dir encoder on
[dirs | pos_out[:, S:]] (a dir MLP of 20 - S inputs), the composite on (B, N, S) densities
(ref_path.render_with_surface, whose per-band form is pinned by the reference's goldens).
Tolerances are those of tests/test_ingp_oracle_gpu.py (TOL, and its max(tol, 4 x oracle
f32 noise) bar on the gradients) and tests/test_extract_gpu.py (1e-2 of the largest sigma).

The hash table is scaled up by 300: a fresh +-1e-4 table gives four near-equal, near-zero
densities, which would hide a swapped band. At 300 the atmosphere renders about 9 % of the
largest colour-map value (oracle, this scene and batch), and exchanging two bands' densities
moves the colour map by far more than the output tolerance (asserted on the oracle in the
train-step test). The factor is bounded above by bf16's 8 significant bits: a per-sample
colour through bf16 layers carries about 2^-8 = 4e-3 relative error, so TOL["bf16"]["out"] =
1e-3 of the largest colour-map value can only hold while the atmosphere's share of it
stays well below 1e-3 / 4e-3 = 25 % (TOL was set on the fresh table, where that share is
~1e-5).

The unfused f16 path returns the loss as an f16 number (losses.py casts it to the colour
map's dtype, as the reference's f16 torch ops do), so its loss can only be held to TOL's
bar up to that rounding: half an f16 ulp, 2^-11 relative, is 16 times the bar of 3e-5.
There the assertion is that the interval oracle loss * (1 +- TOL) contains a value that
rounds to the returned f16 number (_loss_within); every f32 loss is held to TOL as it is."""

import math

import pytest
import torch

import __graft_entry__ as ge
from oracle import ref_ingp, ref_path, ref_tcnn
from tests.test_ingp_oracle_gpu import TOL

pytestmark = pytest.mark.gpu

OPT = {"lr": 1e-2, "betas": [0.9, 0.99], "eps": 1e-15, "weight_decay": 1e-2}
NB = 4
TABLE_SCALE = 300.0


@pytest.fixture(scope="module")
def scene(dev):
    from atmonr_amd.datasets.synthetic import SyntheticHARP2Dataset

    torch.set_num_threads(16)
    return SyntheticHARP2Dataset(n_views=8, img_size=16, device=dev, seed=0)


def _config(n):
    cfg = ge._ingp_config(n)
    cfg.update(multi_band_extinction=True, num_bands=NB)
    return cfg


class RefInstantNGPMultiBand(ref_ingp.RefInstantNGP):
    """Build semantics with multi_band_extinction: S = num_bands density outputs."""

    def __init__(self, cfg, state, scene, half, mlp_half=None, composite="f32"):
        pp = scene.get_point_preprocessor("horizontal")
        super().__init__(cfg, state, ref_ingp.prep_kwargs(pp), scene.scale, scene.max_i,
                         half=half, mlp_half=mlp_half, composite=composite)
        self.S = self.nb

    def _pos_out(self, pts):
        enc = ref_ingp.hashgrid(pts, self.params["pos_encoder"], self.pos_grid, self._rnd)
        return self._mlp(enc, self.params["pos_mlp"], 32, 16, self.ingp["network"],
                         self.mlp_half)

    def forward(self, b, u):
        P, S = self.params, self.S
        B, N = b["origin"].shape[0], self.N
        pts, z = ref_path.sample_uniform_bins(b["origin"], b["dir"], b["len"], u=u, n_bins=N)
        pts = ref_ingp.ref_nerf.preprocess_torch(pts, **self.prep)
        pts = (pts + 1) / 2
        pts = torch.cat([pts[..., :2], pts[..., 2:] / self.alt], dim=-1)
        pos_out = self._pos_out(pts.reshape(B * N, 3))
        dirs = b["dir"][:, None].expand(B, N, 3).reshape(B * N, 3)
        sh = torch.from_numpy(ref_tcnn.sh(dirs.numpy(), 2))
        dir_enc = torch.cat([self._rnd(sh), pos_out[:, S:]], dim=1)  # SH2 | Identity (20 - S)
        color = torch.relu(self._mlp(dir_enc, P["dir_mlp"], 20 - S, self.nb,
                                     self.ingp["rgb_network"], self.mlp_half))
        sigma = torch.relu(pos_out[:, :S])
        ps = (b["origin"] + b["dir"] * b["len"][:, None] + 1) / 2
        surf_sh = self._rnd(torch.from_numpy(ref_tcnn.sh(b["dir"].numpy(), 2)))
        surf_enc = torch.cat([ref_ingp.hashgrid(ps[:, :2], P["surf_encoder"], self.surf_grid,
                                                self._rnd), surf_sh], dim=1)
        color_surf = torch.relu(self._mlp(surf_enc, P["surf_mlp"], 36, self.nb,
                                          self.ingp["surface_network"]))
        ct = torch.float64 if self.composite == "f64" else torch.float32
        cm, alpha, weights, atmo, surf = ref_path.render_with_surface(
            (z * (self.scale / 1000)).to(ct if ct == torch.float64 else z.dtype),
            color.view(B, N, -1).to(ct), sigma.view(B, N, S).to(ct), color_surf.to(ct))
        return {"color_map_fine": cm.double(), "color_map_atmo": atmo.double(),
                "color_map_surf": surf.double(), "weights_fine": weights, "z_vals_fine": z,
                "sigma_fine": sigma.view(B, N, S)[:, :-1],
                "_composite_in": (z * (self.scale / 1000), color.view(B, N, -1).detach(),
                                  sigma.view(B, N, S).detach(), color_surf.detach())}

    @torch.no_grad()
    def sigma(self, pts):
        """instant_ngp.py:208-247 at (P, 3) normalized scene points -> (P, S)."""
        pts = ref_ingp.ref_nerf.preprocess_torch(pts, **self.prep)
        pts = (pts + 1) / 2
        pts = torch.cat([pts[..., :2], pts[..., 2:] / self.alt], dim=-1)
        return torch.clip(self._pos_out(pts.float())[:, :self.S], min=0)


def _state(p):
    return {m: {k: v.detach().clone() for k, v in sd.items()} for m, sd in p.state_dict().items()}


def _pipe(scene, dev, dtype, n=64, fused=True, mlp_dtype=None, seed=5, table_scale=TABLE_SCALE):
    from atmonr_amd.pipelines.instant_ngp import InstantNGPPipeline

    p = InstantNGPPipeline(_config(n), scene, dtype=dtype, fused=fused, seed=seed,
                           mlp_dtype=mlp_dtype)
    p.send_tensors_to(dev)
    sd = _state(p)
    sd["pos_encoder"]["params"] = sd["pos_encoder"]["params"] * table_scale
    p.load_state_dict(sd)  # refreshes the f16 compute copy
    return p


def _rel(a, b):
    return ((a - b).norm() / b.norm().clamp_min(1e-300)).item()


def _loss_within(loss: torch.Tensor, ref: float, tol: float) -> bool:
    """|loss - ref| <= tol |ref| for an f32 loss; for an f16 loss (the unfused f16 path): some
    value of [ref (1 - tol), ref (1 + tol)] rounds to it (module docstring)."""
    if loss.dtype != torch.float16:
        return abs(loss.item() - ref) <= tol * abs(ref)
    lo, hi = (torch.tensor(ref * (1 - k * tol)).half().item() for k in (1, -1))
    return min(lo, hi) <= loss.item() <= max(lo, hi)


@pytest.mark.timeout(600)
@pytest.mark.parametrize("prec,fused", [("f16", True), ("bf16", True), ("f16", False),
                                        ("f32", False)])
def test_multiband_train_step_matches_oracle(scene, dev, prec, fused):
    """One train step, 200 rays x 64 samples, four bands: colour maps, weights, the
    (B, N-1, 4) densities, the loss and every module's gradient. The fused arms fail on the
    code before multi-band (the pipeline left the fused path; bf16 did not construct)."""
    from atmonr_amd.batch_loader import BatchLoader

    B, n = 200, 64
    dtype = torch.float32 if prec == "f32" else torch.float16
    p = _pipe(scene, dev, dtype, n, fused=fused,
              mlp_dtype=torch.bfloat16 if prec == "bf16" else None)
    assert p.fused is fused
    state = _state(p)
    kw = dict(half=prec != "f32", mlp_half="bf16" if prec == "bf16" else None)
    o = RefInstantNGPMultiBand(_config(n), state, scene, **kw)
    batch = next(iter(BatchLoader(scene, B, seed=1)))
    u = torch.rand(B, n, generator=torch.Generator().manual_seed(2))
    res = p.forward(batch, u=u.to(dev))
    loss = p.compute_loss(batch, res)
    loss.backward()
    cb = ref_ingp.cpu_batch(batch)
    ro = o.forward(cb, u)
    lo = o.loss(cb, ro)
    lo.backward()
    tol = TOL[prec]
    assert torch.equal(res["z_vals_fine"].cpu(), ro["z_vals_fine"])
    assert res["sigma_fine"].shape == (B, n - 1, NB)
    sig_o = ro["sigma_fine"].detach()
    # the bands differ visibly: a swapped band cannot hide
    band = sig_o.reshape(-1, NB)
    for i in range(NB):
        for j in range(i + 1, NB):
            assert (band[:, i] - band[:, j]).abs().max() > 0.1 * band.max(), (i, j)
    cmax = ro["color_map_fine"].detach().abs().max()
    # ... nor in the rendering: bands 0 and 1 exchanged move the oracle's colour map by more
    # than ten times the output tolerance
    zs, col_o, sg_o, cs_o = ro["_composite_in"]
    swapped = ref_path.render_with_surface(zs.float(), col_o.float(),
                                           sg_o[..., [1, 0, 2, 3]].float(), cs_o.float())[0]
    swap = ((swapped.double() - ro["color_map_fine"].detach()).abs().max() / cmax).item()
    assert swap > 10 * tol["out"], swap
    rec = {"loss_gpu": loss.item(), "loss_oracle": lo.item(), "sigma_max": band.max().item()}
    for k in ("color_map_fine", "color_map_atmo", "color_map_surf"):
        x, y = res[k].detach().double().cpu(), ro[k].detach().double()
        rec[k] = ((x - y).abs().max() / cmax).item()
    w, wo = res["weights_fine"].detach().double().cpu(), ro["weights_fine"].detach().double()
    assert w.shape == wo.shape
    rec["weights_fine"] = ((w - wo).abs().max() / wo.abs().max()).item()
    rec["sigma_fine"] = ((res["sigma_fine"].detach().double().cpu() - sig_o).abs().max()
                         / sig_o.abs().max()).item()
    rec["loss_rel"] = abs(loss.item() - lo.item()) / abs(lo.item())
    # the oracle's own f32 noise: the same step with an exact (f64) composite
    o64 = RefInstantNGPMultiBand(_config(n), state, scene, composite="f64", **kw)
    o64.loss(cb, o64.forward(cb, u)).backward()
    for m in ref_ingp.MODULES:
        g = getattr(p, m).params.grad.double().cpu()
        rec["grad_" + m] = _rel(g, o.params[m].grad)
        rec["oracle_f32_noise_" + m] = _rel(o.params[m].grad, o64.params[m].grad)
    print(rec)
    for k in ("color_map_fine", "color_map_atmo", "color_map_surf"):
        assert rec[k] <= tol["out"], (k, rec)
    # the densities are one 16-bit MLP's output against its f64 restatement, held to the
    # kernel tests' forward bar, 1e-2 (f16) / 2e-2 (bf16) of the largest value (f32: TOL's
    # output bar). The per-band weights (1 - exp(-sigma delta)) T are linear in sigma at these
    # optical depths, so a relative error of sigma (bf16: 2^-9 = 2e-3 per rounding) is theirs
    # too: the same bar. (TOL's "out" is for the colour maps, of the largest rendered value.)
    field_bar = {"f32": tol["out"], "f16": 1e-2, "bf16": 2e-2}[prec]
    assert rec["weights_fine"] <= field_bar, rec
    assert rec["sigma_fine"] <= field_bar, rec
    assert (loss.dtype == torch.float16) == (prec == "f16" and not fused)
    assert _loss_within(loss.detach(), lo.item(), tol["loss"]), rec
    for m in ref_ingp.MODULES:
        bar = max(tol["grad"], 4 * rec["oracle_f32_noise_" + m])
        assert rec["grad_" + m] <= bar, (m, bar, rec)


def test_multiband_extract(scene, dev):
    """extract on 81 x 64 points: (P, 4), within 1e-2 of the largest oracle value, and bit
    for bit the forward field's sigma on the same coordinates."""
    from atmonr_amd.field import IngpFieldFn
    from atmonr_amd.samplers import preprocess_points

    p = _pipe(scene, dev, torch.float16, 64, seed=9)
    assert p.fused is True
    o = RefInstantNGPMultiBand(_config(64), _state(p), scene, half=True)
    gen = torch.Generator().manual_seed(4)
    col = torch.rand(64, 1, 3, generator=gen) * 1.6 - 0.8
    up = torch.rand(64, 1, 3, generator=gen) * 0.2
    pts = (col + up * torch.linspace(0, 1, 81)[None, :, None]).reshape(-1, 3)
    sigma = p.extract(pts.to(dev).clone(), run_length=81)
    assert sigma.shape == (81 * 64, NB) and bool((sigma >= 0).all())
    ref = o.sigma(pts)
    assert (ref > 0).any(0).all()
    err = (sigma.double().cpu() - ref).abs().max().item()
    print(f"extract: max err {err:.3e} of {ref.abs().max().item():.3e}")
    assert err <= 1e-2 * ref.abs().max().item() + 1e-12, err
    # the forward field on the same hash-grid coordinates (81 samples per "ray")
    coords = preprocess_points(pts.to(dev).clone(), p._prep_ngp).float().contiguous()
    dirs = torch.full((64, 3), 0.5, device=dev)
    with torch.no_grad():
        sig_f, _ = IngpFieldFn.apply(coords, dirs, 81, p.pos_encoder.params, p.pos_mlp.params,
                                     p.dir_mlp.params, p)
    assert sig_f.shape == (81 * 64, NB)
    assert torch.equal(sig_f.to(sigma.dtype), sigma)


def test_multiband_training_reduces_the_loss(scene, dev):
    """30 AdamW steps (batch 256, 64 samples): finite losses and a lower held-out loss; at
    step 0 the fused and the unfused loss agree within twice TOL's f16 loss bar (each is
    within one bar of the oracle; the unfused loss is an f16 number, see _loss_within)."""
    from atmonr_amd.batch_loader import BatchLoader

    p = _pipe(scene, dev, torch.float16, 64)
    q = _pipe(scene, dev, torch.float16, 64, fused=False)
    assert p.fused is True and q.fused is False
    q.load_state_dict(p.state_dict())
    opt = p.get_optimizer(OPT)
    loader = BatchLoader(scene, 256, seed=0)
    held = next(iter(BatchLoader(scene, 512, seed=9)))
    u = torch.full((512, 64), 0.5, device=dev)
    with torch.no_grad():
        before = p.compute_loss(held, p.forward(held, u=u)).item()
        loss_q = q.compute_loss(held, q.forward(held, u=u))
    print(f"step 0: fused {before:.7f} unfused {loss_q.item():.7f}")
    assert loss_q.dtype == torch.float16
    assert _loss_within(loss_q, before, 2 * TOL["f16"]["loss"])
    losses = []
    batches = (b for _ in range(4) for b in loader)  # 8 batches per epoch
    for _, batch in zip(range(30), batches):
        loss = p.compute_loss(batch, p.forward(batch))
        opt.zero_grad()
        loss.backward()
        opt.step()
        losses.append(loss.item())
    with torch.no_grad():
        after = p.compute_loss(held, p.forward(held, u=u)).item()
    print(f"held-out loss {before:.5f} -> {after:.5f}; steps {losses}")
    assert len(losses) == 30 and all(math.isfinite(v) for v in losses)
    assert math.isfinite(after) and after < before


def test_multiband_with_height_fused_equals_unfused(scene, dev):
    """include_height with multi_band_extinction (4-D position grid, point_preprocessor:
    null): the field kernels do not see the grid's dimension, so the combination runs fused.
    One step through both paths on the same parameters: each is within TOL's f16 bars of the
    exact step, so they are within twice those bars of each other."""
    from atmonr_amd.batch_loader import BatchLoader
    from atmonr_amd.pipelines.instant_ngp import InstantNGPPipeline

    cfg = _config(64)
    cfg.update(include_height=True, point_preprocessor=None)
    pipes = []
    for fused in (True, False):
        p = InstantNGPPipeline(cfg, scene, dtype=torch.float16, fused=fused, seed=5)
        p.send_tensors_to(dev)
        assert p.fused is fused
        pipes.append(p)
    a, b = pipes
    sd = _state(a)
    sd["pos_encoder"]["params"] = sd["pos_encoder"]["params"] * TABLE_SCALE
    a.load_state_dict(sd)
    b.load_state_dict(sd)
    batch = next(iter(BatchLoader(scene, 200, seed=1)))
    u = torch.rand(200, 64, device=dev, generator=torch.Generator(device=dev).manual_seed(3))
    ra, rb = a.forward(batch, u=u), b.forward(batch, u=u)
    assert ra["sigma_fine"].shape == rb["sigma_fine"].shape == (200, 63, NB)
    assert ra["norm_heights_fine"].shape == (200, 64)
    cmax = rb["color_map_fine"].float().abs().max()
    tol = TOL["f16"]
    for k in ("color_map_fine", "color_map_atmo", "color_map_surf"):
        err = ((ra[k].float() - rb[k].float()).abs().max() / cmax).item()
        print(k, err)
        assert err <= 2 * tol["out"], (k, err)
    la, lb = a.compute_loss(batch, ra), b.compute_loss(batch, rb)
    assert _loss_within(lb, la.item(), 2 * tol["loss"])
    la.backward()
    lb.backward()
    for m in ref_ingp.MODULES:
        ga, gb = getattr(a, m).params.grad.double(), getattr(b, m).params.grad.double()
        print(m, _rel(ga, gb))
        assert _rel(ga, gb) <= 2 * tol["grad"], m
