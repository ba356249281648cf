"""InstantNGPPipeline with ``include_height: true`` (and ``point_preprocessor: null``)
against the oracle, through the fused and the unfused path.

The oracle is oracle/ref_ingp.RefInstantNGP with a 4-D position grid and a forward that
follows instant_ngp.py:137-206 with the option on: remap, append_heights on the REMAPPED
points (f64 multiply by scale; samplers.py:188), compression of column 2 alone. The height
is restated here in f64 torch (wgs_84.py:83-97); ref_nerf.preprocess_torch clips, so it
cannot serve. Tolerances are those of tests/test_ingp_oracle_gpu.py (TOL, and its
max(tol, 4 x oracle f32 noise) bar on the gradients), tests/test_pipeline_gpu.py (fused
against unfused) and tests/test_extract_gpu.py (1e-2 of the largest sigma); the height
itself within max(one f32 ulp, 1e-9), as tests/test_height_gpu.py derives."""

import math

import numpy as np
import pytest
import torch

import __graft_entry__ as ge
from oracle import ref_ingp, ref_path, ref_tcnn
from tests.test_ingp_oracle_gpu import TOL

pytestmark = pytest.mark.gpu

OPT = {"lr": 1e-2, "betas": [0.9, 0.99], "eps": 1e-15, "weight_decay": 1e-2}
A, B_ = ref_path.WGS_A, ref_path.WGS_B
E, E2 = ref_path.WGS_E, ref_path.WGS_E2


@pytest.fixture(autouse=True)
def _four_primes(monkeypatch):
    monkeypatch.setattr(ref_tcnn, "PRIMES",
                        np.array([1, 2654435761, 805459861, 3674653429], dtype=np.uint32))


@pytest.fixture(scope="module")
def scene(dev):
    from atmonr_amd.datasets.synthetic import SyntheticHARP2Dataset

    torch.set_num_threads(16)
    return SyntheticHARP2Dataset(n_views=8, img_size=16, device=dev, seed=0)


def _config(n, include_height=True):
    cfg = ge._ingp_config(n)
    cfg.update(include_height=include_height, point_preprocessor=None)
    return cfg


def _altitude(xyz: torch.Tensor) -> torch.Tensor:
    """cartesian_to_horizontal's ellipsoidal height (wgs_84.py:83-97), f64."""
    x, y, z = xyz[..., 0], xyz[..., 1], xyz[..., 2]
    lon = torch.atan2(y, x)
    D = torch.sqrt(x ** 2 + y ** 2)
    u = torch.atan2(z / D, torch.zeros_like(x) + A / B_)
    lat = torch.atan2(z + (E2 * B_) * (torch.sin(u) ** 3), D - (E * A) * (torch.cos(u) ** 3))
    N = A / torch.sqrt(1 - (E * torch.sin(lat) ** 2))
    return x / (torch.cos(lat) * torch.cos(lon)) - N


class RefInstantNGPHeight(ref_ingp.RefInstantNGP):
    """Build semantics with include_height: the 4-D position grid and the reference's
    order of remap, height and compression."""

    def __init__(self, cfg, state, scene, half, composite="f32"):
        super().__init__(cfg, state, {}, scene.scale, scene.max_i, half=half,
                         composite=composite)
        self.pos_grid = ref_ingp._grid_cfg(self.ingp["encoding"], 4)
        self.offset = torch.as_tensor(scene.offset).double().cpu()
        self.roh = float(scene.config["ray_origin_height"])

    def coords(self, pts):
        """(..., 3) normalized points, f32 or f64 -> (..., 4) hash-grid coordinates."""
        pts = (pts + 1) / 2
        h = (_altitude(pts.double() * self.scale + self.offset) / self.roh).float()
        pts = torch.cat([pts, h[..., None]], dim=-1)  # f64 points promote the height
        return torch.cat([pts[..., :2], pts[..., 2:3] / self.alt, pts[..., 3:]], dim=-1)

    def forward(self, b, u):
        P = self.params
        B, N = b["origin"].shape[0], self.N
        pts, z = ref_path.sample_uniform_bins(b["origin"], b["dir"], b["len"], u=u, n_bins=N)
        pts = self.coords(pts)
        pos_enc = ref_ingp.hashgrid(pts.reshape(B * N, 4), P["pos_encoder"], self.pos_grid,
                                    self._rnd)
        pos_out = self._mlp(pos_enc, P["pos_mlp"], 32, 16, self.ingp["network"], self.mlp_half)
        dirs = b["dir"][:, None].expand(B, N, 3).reshape(B * N, 3)
        sh = torch.from_numpy(ref_tcnn.sh(dirs.numpy(), 2))
        dir_enc = torch.cat([self._rnd(sh), pos_out[:, 1:]], dim=1)
        color = torch.relu(self._mlp(dir_enc, P["dir_mlp"], 19, self.nb,
                                     self.ingp["rgb_network"], self.mlp_half))
        sigma = torch.relu(pos_out[:, :1])
        ps = (b["origin"] + b["dir"] * b["len"][:, None] + 1) / 2
        surf_sh = self._rnd(torch.from_numpy(ref_tcnn.sh(b["dir"].numpy(), 2)))
        surf_enc = torch.cat([ref_ingp.hashgrid(ps[:, :2], P["surf_encoder"], self.surf_grid,
                                                self._rnd), surf_sh], dim=1)
        color_surf = torch.relu(self._mlp(surf_enc, P["surf_mlp"], 36, self.nb,
                                          self.ingp["surface_network"]))
        ct = torch.float64 if self.composite == "f64" else torch.float32
        cm, alpha, weights, atmo, surf = ref_path.render_with_surface(
            (z * (self.scale / 1000)).to(ct if ct == torch.float64 else z.dtype),
            color.view(B, N, -1).to(ct), sigma.view(B, N, 1).to(ct), color_surf.to(ct))
        return {"color_map_fine": cm.double(), "color_map_atmo": atmo.double(),
                "color_map_surf": surf.double(), "weights_fine": weights, "z_vals_fine": z,
                "norm_heights_fine": pts[..., 3]}

    @torch.no_grad()
    def sigma(self, pts):
        """instant_ngp.py:208-247 at (P, 3) points."""
        enc = ref_ingp.hashgrid(self.coords(pts), self.params["pos_encoder"], self.pos_grid,
                                self._rnd)
        pos_out = self._mlp(enc, self.params["pos_mlp"], 32, 16, self.ingp["network"],
                            self.mlp_half)
        return torch.clip(pos_out[:, :1], min=0)


def _pipe(scene, dev, dtype, n, fused=True, include_height=True, seed=5):
    from atmonr_amd.pipelines.instant_ngp import InstantNGPPipeline

    p = InstantNGPPipeline(_config(n, include_height), scene, dtype=dtype, fused=fused,
                           seed=seed)
    p.send_tensors_to(dev)
    return p


def _state(p):
    return {m: {k: v.detach().clone() for k, v in sd.items()} for m, sd in p.state_dict().items()}


def _rel(a, b):
    return ((a - b).norm() / b.norm().clamp_min(1e-300)).item()


def _check_heights(h, h_ref):
    h, ref = h.detach().double().cpu().numpy(), h_ref.detach().float().cpu().numpy()
    bound = np.maximum(np.spacing(np.abs(ref)).astype(np.float64), 1e-9)
    err = np.abs(h - ref.astype(np.float64))
    print(f"norm_heights_fine: max err {err.max():.3e}, range {ref.min():.3f} .. {ref.max():.3f}")
    assert np.all(err <= bound), err.max()


@pytest.mark.timeout(600)
@pytest.mark.parametrize("prec,n_samples,B", [("f32", 64, 200), ("f16", 64, 200),
                                              ("f32", 1024, 24), ("f16", 1024, 24)])
def test_train_step_with_height_matches_oracle(scene, dev, prec, n_samples, B):
    from atmonr_amd.batch_loader import BatchLoader

    p = _pipe(scene, dev, torch.float32 if prec == "f32" else torch.float16, n_samples)
    state = _state(p)
    o = RefInstantNGPHeight(_config(n_samples), state, scene, half=prec == "f16")
    batch = next(iter(BatchLoader(scene, B, seed=1)))
    u = torch.rand(B, n_samples, generator=torch.Generator().manual_seed(2))
    res = p.forward(batch, u=u.to(dev))
    loss = p.compute_loss(batch, res)
    loss.backward()
    cb = ref_ingp.cpu_batch(batch)
    ro = o.forward(cb, u)
    lo = o.loss(cb, ro)
    lo.backward()
    tol = TOL[prec]
    assert torch.equal(res["z_vals_fine"].cpu(), ro["z_vals_fine"])
    assert res["norm_heights_fine"].shape == (B, n_samples)
    _check_heights(res["norm_heights_fine"], ro["norm_heights_fine"])
    cmax = ro["color_map_fine"].detach().abs().max()
    rec = {"loss_gpu": loss.item(), "loss_oracle": lo.item()}
    for k in ("color_map_fine", "color_map_atmo", "color_map_surf"):
        x, y = res[k].detach().double().cpu(), ro[k].detach().double()
        rec[k] = ((x - y).abs().max() / cmax).item()
    rec["loss_rel"] = abs(loss.item() - lo.item()) / abs(lo.item())
    # the oracle's own f32 noise: the same step with an exact (f64) composite
    o64 = RefInstantNGPHeight(_config(n_samples), state, scene, half=prec == "f16",
                              composite="f64")
    o64.loss(cb, o64.forward(cb, u)).backward()
    for m in ref_ingp.MODULES:
        g = getattr(p, m).params.grad.double().cpu()
        rec["grad_" + m] = _rel(g, o.params[m].grad)
        rec["oracle_f32_noise_" + m] = _rel(o.params[m].grad, o64.params[m].grad)
    print(rec)
    for k in ("color_map_fine", "color_map_atmo", "color_map_surf"):
        assert rec[k] <= tol["out"], (k, rec)
    assert rec["loss_rel"] <= tol["loss"], rec
    for m in ref_ingp.MODULES:
        bar = max(tol["grad"], 4 * rec["oracle_f32_noise_" + m])
        assert rec["grad_" + m] <= bar, (m, bar, rec)


@pytest.mark.parametrize("include_height", [True, False])
def test_fused_equals_unfused_without_a_preprocessor(scene, dev, include_height):
    """point_preprocessor: null through both paths, with the height (mode 2 of the sampler
    kernel against anr_append_heights) and without it (mode 0), on the same step."""
    from atmonr_amd.batch_loader import BatchLoader

    a = _pipe(scene, dev, torch.float32, 64, fused=True, include_height=include_height)
    b = _pipe(scene, dev, torch.float32, 64, fused=False, include_height=include_height)
    b.load_state_dict(a.state_dict())
    batch = next(iter(BatchLoader(scene, 300, seed=1)))
    u = torch.rand(300, 64, device=dev, generator=torch.Generator(device=dev).manual_seed(3))
    ra, rb = a.forward(batch, u=u), b.forward(batch, u=u)
    for k in ("color_map_fine", "color_map_atmo", "color_map_surf", "weights_fine"):
        x, y = ra[k].float(), rb[k].float()
        assert (x - y).abs().max() <= 1e-4 * y.abs().max() + 1e-6, k
    assert torch.equal(ra["z_vals_fine"], rb["z_vals_fine"])
    assert ("norm_heights_fine" in ra) == include_height == ("norm_heights_fine" in rb)
    if include_height:
        assert ra["norm_heights_fine"].shape == (300, 64)
        assert torch.equal(ra["norm_heights_fine"], rb["norm_heights_fine"])
    la, lb = a.compute_loss(batch, ra), b.compute_loss(batch, rb)
    la.backward()
    lb.backward()
    for m in ("pos_encoder", "pos_mlp", "dir_mlp", "surf_encoder", "surf_mlp"):
        ga, gb = getattr(a, m).params.grad, getattr(b, m).params.grad
        assert (ga - gb).abs().max() <= 1e-3 * gb.abs().max() + 1e-9, m


@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("f64", [False, True])
def test_extract_with_height_matches_oracle(scene, dev, fused, f64):
    """81 altitudes x 64 columns of normalized scene points, f32 and f64 (the extract
    script's): sigma within 1e-2 of the largest value (f16 kernels), as test_extract_gpu."""
    p = _pipe(scene, dev, torch.float16, 64, fused=fused, seed=9)
    gen = torch.Generator().manual_seed(4)
    with torch.no_grad():  # a table with structure: the initial +-1e-4 gives a flat field
        p.pos_encoder.params.copy_((torch.rand(p.pos_encoder.params.shape, generator=gen) - 0.5)
                                   .to(dev))
    o = RefInstantNGPHeight(_config(64), _state(p), scene, half=True)
    col = torch.rand(64, 1, 3, generator=gen, dtype=torch.float64) * 1.6 - 0.8
    up = torch.rand(64, 1, 3, generator=gen, dtype=torch.float64) * 0.2
    pts = (col + up * torch.linspace(0, 1, 81, dtype=torch.float64)[None, :, None]).reshape(-1, 3)
    pts = pts if f64 else pts.float()
    sigma = p.extract(pts.to(dev).clone(), run_length=81)
    assert sigma.shape == (81 * 64, 1) and bool((sigma >= 0).all())
    ref = o.sigma(pts)
    assert (ref > 0).any()
    err = (sigma.double().cpu() - ref).abs().max().item()
    print(f"extract: max err {err:.3e} of {ref.abs().max().item():.3e}")
    assert err <= 1e-2 * ref.abs().max().item() + 1e-12, err


def test_training_with_height_reduces_the_loss(scene, dev):
    from atmonr_amd.batch_loader import BatchLoader

    p = _pipe(scene, dev, torch.float16, 64)
    opt = p.get_optimizer(OPT)
    loader = BatchLoader(scene, 256, seed=0)
    held = next(iter(BatchLoader(scene, 512, seed=9)))
    u = torch.full((512, 64), 0.5, device=dev)
    with torch.no_grad():
        before = p.compute_loss(held, p.forward(held, u=u)).item()
    losses = []
    for _, batch in zip(range(8), loader):
        loss = p.compute_loss(batch, p.forward(batch))
        opt.zero_grad()
        loss.backward()
        opt.step()
        losses.append(loss.item())
    with torch.no_grad():
        after = p.compute_loss(held, p.forward(held, u=u)).item()
    print(f"held-out loss {before:.5f} -> {after:.5f}; steps {losses}")
    assert len(losses) == 8 and all(math.isfinite(v) for v in losses)
    assert math.isfinite(after) and after < before
