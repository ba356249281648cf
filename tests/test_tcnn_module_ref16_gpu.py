"""atmonr_amd.tcnn modules with ``loss_scale`` (tinycudann's per-call loss-scaled f16
backward) and InstantNGPPipeline(fused=False, numerics="reference") against the oracle's
``_TcnnCall`` (oracle/ref_ingp.py), on the GPU.

1. anr_grad_quantize_add_f16 equals quantise-then-add bit for bit, at every alignment.
2. Network, 3. HashGrid encodings, 4. the Composite dir encoder's input gradient: one module
   call against ``_TcnnCall`` over the restated module.
5. Two calls of one module in one graph round their gradients separately.
6. The unfused reference pipeline against the oracle in reference semantics, live field; the
   fused reference pipeline beside it (recorded).
7. The bare ``import atmonr_amd.tcnn as tcnn`` swap plus ``tcnn.reference_numerics()``: the
   reference's six constructions and its forward in torch's own f16 ops, against the two
   restatements of torch's f16 kernels the oracle has (ref_acc "cuda" and "cpu").

With ANR_TCNN_MODULE_OUT set, the records of 6 and 7 are written there as JSON.
"""

import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import __graft_entry__ as ge
from oracle import ref_f16, ref_ingp

pytestmark = pytest.mark.gpu

LS = 128.0
# TOL["ref16"] of tests/test_ingp_oracle_gpu.py
TOL = {"out": 1e-5, "loss": 1e-5, "grad": 3e-4}
N_SAMPLES, N_RAYS = 64, 40
_REC = {}


def _dump():
    out = os.environ.get("ANR_TCNN_MODULE_OUT")
    if out:
        os.makedirs(os.path.dirname(out) or ".", exist_ok=True)
        with open(out, "w") as f:
            json.dump(_REC, f, indent=1)


def _rel(a: torch.Tensor, b: torch.Tensor) -> float:
    return ((a - b).norm() / b.norm().clamp_min(1e-300)).item()


def _f16_steps(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """How many f16 numbers apart two f16 tensors are, element by element."""
    def key(t):
        assert t.dtype == torch.float16
        i = t.detach().cpu().contiguous().view(torch.int16).to(torch.int64)
        return torch.where(i >= 0, i, -(i & 0x7FFF))
    return (key(a) - key(b)).abs()


def _f16_representable(t: torch.Tensor) -> torch.Tensor:
    t = t.detach().double().cpu()
    return t.half().double() == t


def _dout(M: int, C: int, seed: int) -> torch.Tensor:
    """f16 gradient rows of mixed magnitude, every third 32-row block zeroed."""
    g = torch.Generator().manual_seed(seed)
    d = torch.randn(M, C, generator=g) * torch.exp(-12.0 * torch.rand(M, C, generator=g))
    d[(torch.arange(M) // 32) % 3 == 2] = 0
    return d.half()


# ------------------------------------------------------------------ 1. the kernel
@pytest.mark.parametrize("off", [0, 1])
@pytest.mark.parametrize("n", [0, 1, 3, 4, 7, 4096 + 3])
def test_grad_quantize_add(dev, n, off):
    from atmonr_amd import _lib

    rng = np.random.default_rng(100 * n + off)
    pad = 8
    sc = (rng.standard_normal(n + 2 * pad) *
          np.exp(rng.uniform(-25, 5, n + 2 * pad))).astype(np.float32)
    planted = [-0.0, 600.0, -600.0, 0.0, 0.0]
    for k in range(min(n, len(planted))):  # head elements ...
        sc[off + k] = planted[k]
    if n > 2 * len(planted):               # ... and tail elements
        for k, v in enumerate(planted):
            sc[off + n - 1 - k] = v
    gr = rng.standard_normal(n + 2 * pad).astype(np.float32)
    ts, tg = torch.from_numpy(sc).to(dev), torch.from_numpy(gr).to(dev)
    _lib.call("anr_grad_quantize_add_f16", ts.data_ptr() + 4 * off, tg.data_ptr() + 4 * off, n,
              LS, _lib.stream(dev))
    g = sc[off:off + n]
    with np.errstate(over="ignore"):
        want = (ref_f16.h(g * np.float32(128)).astype(np.float16) /
                np.float16(128)).astype(np.float32)
    if n > 2 * len(planted):
        assert np.isinf(want).any() and (want == 0).any()  # overflow and underflow reached
    exp_g, exp_s = gr.copy(), sc.copy()
    exp_g[off:off + n] = gr[off:off + n] + want
    exp_s[off:off + n] = 0.0
    assert np.array_equal(tg.cpu().numpy(), exp_g)
    got_s = ts.cpu().numpy()
    assert np.array_equal(got_s, exp_s)
    assert not np.signbit(got_s[off:off + n]).any()  # +0, the scatter's neutral element


def test_grad_quantize_add_equals_the_composition(dev):
    """Scratch aligned, gradient at every element offset of a bucket (and the reverse)."""
    from atmonr_amd import _lib

    rng = np.random.default_rng(9)
    n = 1000
    sc = (rng.standard_normal(n) * np.exp(rng.uniform(-25, 5, n))).astype(np.float32)
    gr = rng.standard_normal(n).astype(np.float32)
    want = torch.from_numpy(sc).to(dev)
    _lib.call("anr_grad_quantize_f16", want.data_ptr(), n, LS, _lib.stream(dev))
    want = torch.from_numpy(gr).to(dev) + want
    for so, go in [(0, 0), (0, 1), (0, 2), (0, 3), (1, 0), (3, 2)]:
        ts, tg = torch.zeros(n + 4, device=dev), torch.zeros(n + 4, device=dev)
        ts[so:so + n] = torch.from_numpy(sc).to(dev)
        tg[go:go + n] = torch.from_numpy(gr).to(dev)
        _lib.call("anr_grad_quantize_add_f16", ts.data_ptr() + 4 * so, tg.data_ptr() + 4 * go, n,
                  LS, _lib.stream(dev))
        assert torch.equal(tg[go:go + n], want), (so, go)
        assert not ts.any() and not tg[:go].any() and not tg[go + n:].any(), (so, go)


# ------------------------------------------------------------------ 2. Network, per call
def _net_cfg(width, n_hidden):
    return {"otype": "FullyFusedMLP", "activation": "ReLU", "output_activation": "None",
            "n_neurons": width, "n_hidden_layers": n_hidden}


@pytest.mark.parametrize("n_in,n_out,width,n_hidden", [(32, 16, 32, 1), (19, 4, 32, 2),
                                                        (36, 4, 64, 2)])
def test_network_call_matches_tcnn_call(dev, n_in, n_out, width, n_hidden):
    from atmonr_amd import tcnn

    M = 200
    net = tcnn.Network(n_in, n_out, _net_cfg(width, n_hidden), seed=11, loss_scale=LS).to(dev)
    x = torch.randn(M, n_in, generator=torch.Generator().manual_seed(1)).half()
    dout = _dout(M, n_out, 2)
    xg = x.to(dev).requires_grad_()
    y = net(xg)
    assert y.dtype == torch.float16
    y.backward(dout.to(dev))
    xo = x.clone().requires_grad_()
    po = net.params.detach().cpu().double().requires_grad_()
    yo = ref_ingp._TcnnCall.apply(xo, po, lambda a, p: ref_ingp._mlp_ref(
        a, p, n_in, n_out, width, n_hidden, "f64"))
    yo.backward(dout)
    g = net.params.grad
    assert g.dtype == torch.float32 and xg.grad.dtype == torch.float16
    assert _f16_representable(g * LS).all()
    gp, gx = _rel(g.double().cpu(), po.grad), _rel(xg.grad.double().cpu(), xo.grad.double())
    print("network", (n_in, n_out, width, n_hidden), "grad params", gp, "input", gx)
    assert po.grad.norm() > 0 and xo.grad.norm() > 0
    assert gp <= TOL["grad"] and gx <= TOL["grad"], (gp, gx)
    assert torch.equal((xg.grad.cpu() == 0).all(1), (xo.grad == 0).all(1))


# ------------------------------------------------------------------ 3. HashGrid, per call
def _points(M, d, seed):
    x = torch.rand(M, d, generator=torch.Generator().manual_seed(seed))
    x[M - 40:] = x[:40]  # repeated points: cells collect sums
    return x


def _half_then_double(t):
    return t.half().double()


@pytest.mark.parametrize("which", ["pos_grid", "surface_composite"])
def test_hashgrid_call_matches_tcnn_call(dev, which):
    from atmonr_amd import tcnn

    M = 200
    ingp = ge._ingp_config(64)["instant_ngp"]
    if which == "pos_grid":
        d, cfg = 3, ingp["encoding"]
        grid = ref_ingp._grid_cfg(cfg, 3)

        def fn(a, p):
            return ref_ingp.hashgrid(a, p, grid, _half_then_double, "f64")
    else:
        d, cfg = 5, ingp["surface_encoding"]
        grid = ref_ingp._grid_cfg(cfg["nested"][0], 2)

        def fn(a, p):
            return torch.cat([ref_ingp.hashgrid(a[:, :2], p, grid, _half_then_double, "f64"),
                              ref_ingp._sh2(a[:, 2:5])], dim=1)
    enc = tcnn.Encoding(d, cfg, seed=21, loss_scale=LS).to(dev)
    x = _points(M, d, 3)
    dout = _dout(M, enc.n_output_dims, 4)
    y = enc(x.to(dev))
    assert y.dtype == torch.float16
    y.backward(dout.to(dev))
    po = enc.params.detach().cpu().double().requires_grad_()
    yo = ref_ingp._TcnnCall.apply(x, po, fn)
    yo.backward(dout)
    g = enc.params.grad
    assert g.dtype == torch.float32
    assert _f16_representable(g * LS).all()
    gp = _rel(g.double().cpu(), po.grad)
    print("hashgrid", which, "grad params", gp, "nonzero", int((po.grad != 0).sum()))
    assert po.grad.norm() > 0
    assert gp <= TOL["grad"], gp
    assert not g.cpu()[po.grad == 0].any()
    # the module's scratch is left zeroed for its next call
    assert not enc._grad_scratch.any()


# ------------------------------------------------------------------ 4. dir encoder dL/dx
def test_dir_encoder_input_gradient(dev):
    from atmonr_amd import tcnn

    M = 200
    enc = tcnn.Encoding(19, ge._ingp_config(64)["instant_ngp"]["dir_encoding"],
                        loss_scale=LS).to(dev)
    gen = torch.Generator().manual_seed(5)
    dirs = torch.rand(M, 3, generator=gen).to(dev)
    leaf = torch.rand(M, 16, generator=gen).to(dev).requires_grad_()
    dout = (torch.randn(M, 4 + 16, generator=gen) * 0.1).half()
    dout[5, 4 + 2] = 600.0
    dout[7, 4 + 9] = 2.0 ** -24
    y = enc(torch.cat([dirs.detach(), leaf], dim=1))
    assert y.dtype == torch.float16 and y.shape == (M, 20)
    y.backward(dout.to(dev))
    g = leaf.grad.cpu()
    assert g.dtype == torch.float32
    want = dout[:, 4:].float()
    assert g[5, 2] == float("inf")  # f16(600 * 128) overflows, as in tinycudann
    want[5, 2] = float("inf")
    assert g[7, 9] == 2.0 ** -24
    assert torch.equal(g, want)


# ------------------------------------------------------------------ 5. two calls, one graph
def test_two_calls_round_separately(dev):
    from atmonr_amd import tcnn

    M = 200
    net = tcnn.Network(32, 16, _net_cfg(32, 1), seed=11, loss_scale=LS).to(dev)
    gen = torch.Generator().manual_seed(6)
    x1, x2 = (torch.randn(M, 32, generator=gen).half().to(dev) for _ in range(2))
    g1 = torch.randn(M, 16, generator=gen).half().to(dev)
    g2 = (torch.randn(M, 16, generator=gen) * 2.0 ** -6).half().to(dev)
    q = []
    for x, g in ((x1, g1), (x2, g2)):
        net.params.grad = None
        net(x).backward(g)
        q.append(net.params.grad.clone())
    net.params.grad = None
    ((net(x1) * g1).sum() + (net(x2) * g2).sum()).backward()
    want = q[0] + q[1]
    assert torch.equal(net.params.grad, want)
    assert all(_f16_representable(t * LS).all() for t in q)
    # the sum of two rounded gradients needs more bits than one f16: rounded per call, not
    # after the sum
    assert not _f16_representable(want * LS).all()
    # a third call adds into the existing .grad (no fresh buffer), rounded on its own
    net(x1).backward(g1)
    assert torch.equal(net.params.grad, want + q[0])


# ------------------------------------------------------------------ 6 / 7. the pipeline
@pytest.fixture(scope="module")
def scene(dev):
    from atmonr_amd.datasets.synthetic import SyntheticHARP2Dataset

    torch.set_num_threads(min(16, os.cpu_count() or 1))
    return SyntheticHARP2Dataset(n_views=8, img_size=16, device=dev, seed=0)


def _pair(scene, dev, fused, table_scale=10.0, state=None):
    """The pipeline in reference numerics (seed 5, hash table scaled by ``table_scale`` so
    that the f16 composite's dL/dcolor is alive), or one loaded from ``state``."""
    from atmonr_amd.pipelines.instant_ngp import InstantNGPPipeline

    p = InstantNGPPipeline(ge._ingp_config(N_SAMPLES), scene, dtype=torch.float16, fused=fused,
                           seed=5, numerics="reference")
    p.send_tensors_to(dev)
    if state is None:
        state = {m: {k: v.detach().clone() for k, v in s.items()}
                 for m, s in p.state_dict().items()}
        state["pos_encoder"]["params"] = state["pos_encoder"]["params"] * float(table_scale)
    p.load_state_dict(state)
    return p, state


def _oracle(scene, state, scale, acc="f64", ref_acc="cuda"):
    pp = scene.get_point_preprocessor("horizontal")
    return ref_ingp.RefInstantNGP(ge._ingp_config(N_SAMPLES), state, ref_ingp.prep_kwargs(pp),
                                  scale, scene.max_i, half=True, semantics="reference",
                                  acc=acc, ref_acc=ref_acc)


MAPS = ("color_map_fine", "color_map_atmo", "color_map_surf")


@pytest.fixture(scope="module")
def shared(scene, dev):
    """The unfused reference pipeline's state, one batch and draws, and the oracle's arms on
    them: A = f64 sums with torch's CUDA f16 accumulation, its f32 / f32rev summation arms,
    and C = torch's CPU f16 kernels."""
    from atmonr_amd.batch_loader import BatchLoader

    p, state = _pair(scene, dev, fused=False)
    batch = next(iter(BatchLoader(scene, N_RAYS, seed=1)))
    u = torch.rand(N_RAYS, N_SAMPLES, generator=torch.Generator().manual_seed(2))
    cb = ref_ingp.cpu_batch(batch)
    arms = {}
    for name, acc, ref_acc in (("A", "f64", "cuda"), ("f32", "f32", "cuda"),
                               ("f32rev", "f32rev", "cuda"), ("C", "f64", "cpu")):
        o = _oracle(scene, state, p.scale, acc, ref_acc)
        ro = o.forward(cb, u)
        lo = o.loss(cb, ro)
        lo.backward()
        arms[name] = {"res": {k: v.detach() for k, v in ro.items()}, "loss": lo.detach(),
                      "grad": {m: o.params[m].grad for m in ref_ingp.MODULES}}
    A = arms["A"]["grad"]
    spread = {m: max(_rel(arms[a]["grad"][m], A[m]) for a in ("f32", "f32rev"))
              for m in ref_ingp.MODULES}
    return {"p": p, "state": state, "batch": batch, "u": u, "arms": arms, "spread": spread}


def _step(p, batch, u, dev):
    for m in p.modules():
        m.params.grad = None
    res = p.forward(batch, u=u.to(dev))
    loss = p.compute_loss(batch, res)
    loss.backward()
    torch.cuda.synchronize(dev)
    return res, loss


def test_unfused_reference_pipeline_matches_oracle(scene, dev, shared):
    """One train step of InstantNGPPipeline(fused=False, numerics="reference") against the
    oracle in reference semantics (arm A), and the fused reference pipeline from the same
    state beside it (recorded only: another MFMA accumulation order).

    Measured on MI355X (profiles/tcnn_module_ref16.json): colour maps and loss bit-exact,
    no zero rays; gradients, relative L2 (4 x arm spread in brackets): pos_encoder 3.1e-5
    (8.6e-4), pos_mlp 1.6e-5 (5.6e-4), dir_mlp 0 (6.0e-4), surf_encoder 1.3e-4 (2.8e-3),
    surf_mlp 5.6e-6 (1.5e-3). Fused against unfused: loss equal, one colour-map entry of
    160 one f16 step apart, color_fine up to 3 steps in 0.14 % of the entries, the hash
    table's gradient 1.5e-6 apart and every other module's identical."""
    p, batch, u = shared["p"], shared["batch"], shared["u"]
    A, spread = shared["arms"]["A"], shared["spread"]
    assert p.fused is False and all(m.loss_scale == LS for m in p.modules())
    res, loss = _step(p, batch, u, dev)
    ro, lo = A["res"], A["loss"]
    rec = {"loss_gpu": loss.item(), "loss_oracle": lo.item(), "arm_spread": spread,
           "zero_rays": p.zero_rays_total}
    cmax = ro["color_map_fine"].double().abs().max()
    for k in MAPS:
        x, y = res[k].detach().double().cpu(), ro[k].double()
        rec[k] = ((x - y).abs().max() / cmax).item()
        rec[k + "_max_f16_steps"] = int(_f16_steps(res[k], ro[k]).max().item())
    rec["loss_rel"] = abs(loss.item() - lo.item()) / abs(lo.item())
    grads = {m: getattr(p, m).params.grad.detach().clone() for m in ref_ingp.MODULES}
    for m in ref_ingp.MODULES:
        g = grads[m].double().cpu()
        rec["grad_" + m] = _rel(g, A["grad"][m])
        rec["grad_zero_same_" + m] = bool(torch.equal(g == 0, A["grad"][m] == 0))
        rec["grad_x128_f16_" + m] = bool(_f16_representable(grads[m] * LS).all())
    # ---- the fused reference pipeline from the same state on the same batch (recorded)
    pf, _ = _pair(scene, dev, fused=True, state=shared["state"])
    rf, lf = _step(pf, batch, u, dev)
    fused = {"loss_f16_steps": int(_f16_steps(lf.reshape(1), loss.reshape(1)).item())}
    for k in MAPS + ("sigma_fine", "color_fine"):
        st = _f16_steps(rf[k], res[k])
        fused[k + "_max_f16_steps"] = int(st.max().item())
        fused[k + "_differ_frac"] = (st != 0).double().mean().item()
    for m in ref_ingp.MODULES:
        fused["grad_" + m] = _rel(getattr(pf, m).params.grad.double().cpu(),
                                  grads[m].double().cpu())
    rec["fused_vs_unfused"] = fused
    _REC["unfused_reference_vs_oracle"] = rec
    _dump()
    print("unfused reference pipeline", rec)
    # ---- exact
    assert torch.equal(res["z_vals_fine"].cpu(), ro["z_vals_fine"])
    assert rec["zero_rays"] == 0
    assert res["color_map_fine"].dtype == torch.float16 and loss.dtype == torch.float16
    # ---- tolerances
    assert A["grad"]["dir_mlp"].norm() > 0  # the field is alive
    for k in MAPS:
        assert rec[k] <= TOL["out"], (k, rec)
    assert rec["loss_rel"] <= TOL["loss"], rec
    for m in ref_ingp.MODULES:
        bar = max(TOL["grad"], 4 * spread[m])
        assert rec["grad_" + m] <= bar, (m, bar, rec)
    for m in ("pos_mlp", "dir_mlp", "surf_mlp"):
        assert rec["grad_zero_same_" + m], (m, rec)


def _beer_lambert_f16(z_km, color, sigma, color_surf):
    """The Beer-Lambert composite with a surface term, in torch's own f16 ops: bin widths
    between the midpoints of the f16 depths (the first bin from 0, the last to the last
    depth), alpha = 1 - exp(-sigma * width), transmittance as the exclusive cumprod of
    1 - alpha + 1e-10, the surface seen through the product of every 1 - alpha."""
    z = z_km.to(color.dtype)
    mids = (z[:, 1:] + z[:, :-1]) / 2
    edges = torch.cat([z[:, :1] * 0, mids, z[:, -1:]], dim=1)
    width = (edges[:, 1:] - edges[:, :-1])[..., None]
    alpha = 1 - torch.exp(-sigma * width)
    one = torch.ones_like(alpha[:, :1])
    trans = torch.cumprod(torch.cat([one, 1 - alpha + 1e-10], dim=1), dim=1)[:, :-1]
    atmo = (color * (alpha * trans)).sum(dim=1)
    surf = (1 - alpha).prod(dim=1) * color_surf
    return atmo + surf, atmo, surf


def _mse_plus_hdr(pred, gt, max_i):
    eps = 1e-3 * max_i
    return (F.mse_loss(pred / max_i, gt / max_i) +
            0.2 * F.mse_loss(torch.log(gt + eps), torch.log(pred + eps)))


def test_bare_import_swap_under_torch_f16_ops(scene, dev, shared):
    """``import atmonr_amd.tcnn as tcnn`` plus ``tcnn.reference_numerics()``,
    the reference's six constructions and its forward, composite and loss as plain torch
    ops on the f16 module outputs."""
    import atmonr_amd.tcnn as tcnn
    from atmonr_amd.samplers import sample_uniform_bins

    cfg = ge._ingp_config(N_SAMPLES)
    ingp, nb, N = cfg["instant_ngp"], cfg["num_bands"], N_SAMPLES
    tcnn.reference_numerics()
    try:
        mods = {}
        mods["pos_encoder"] = tcnn.Encoding(3, ingp["encoding"])
        mods["pos_mlp"] = tcnn.Network(mods["pos_encoder"].n_output_dims, 16, ingp["network"])
        mods["dir_encoder"] = tcnn.Encoding(3 + 16 - 1, ingp["dir_encoding"])
        mods["dir_mlp"] = tcnn.Network(mods["dir_encoder"].n_output_dims, nb,
                                       ingp["rgb_network"])
        mods["surf_encoder"] = tcnn.Encoding(2 + 3, ingp["surface_encoding"])
        mods["surf_mlp"] = tcnn.Network(mods["surf_encoder"].n_output_dims, nb,
                                        ingp["surface_network"])
    finally:
        tcnn.reference_numerics(False)
    for name, m in mods.items():
        assert m.loss_scale == LS, name
        m.load_state_dict(shared["state"][name])
        m.to(dev)
    batch, u = shared["batch"], shared["u"].to(dev)
    pp = scene.get_point_preprocessor(cfg["point_preprocessor"])
    B = batch["origin"].shape[0]
    pts, z_vals = sample_uniform_bins(batch, N, u=u)
    pts_surf = batch["origin"] + batch["dir"] * batch["len"][:, None]
    pts = (pp(pts) + 1) / 2
    pts_surf = (pts_surf + 1) / 2
    dirs = batch["dir"][:, None].repeat(1, N, 1)
    pts[..., 2] = pts[..., 2] / cfg["alt_compress_factor"]
    pos_out = mods["pos_mlp"](mods["pos_encoder"](pts.view(B * N, -1)))
    dir_in = torch.cat([dirs.view(B * N, 3), pos_out[:, 1:]], dim=1)
    assert dir_in.dtype == torch.float32
    color = mods["dir_mlp"](mods["dir_encoder"](dir_in)).view(B, N, nb)
    color_surf = mods["surf_mlp"](mods["surf_encoder"](
        torch.cat([pts_surf[:, :2], dirs[:, 0]], dim=1)))
    sigma = pos_out[..., :1].view(B, N, -1)
    color, color_surf, sigma = F.relu(color), F.relu(color_surf), F.relu(sigma)
    assert color.dtype == sigma.dtype == color_surf.dtype == torch.float16
    scale = shared["p"].scale
    cm, atmo, surf = _beer_lambert_f16(z_vals * (scale / 1000), color, sigma, color_surf)
    pred = torch.take_along_dim(cm, batch["irgb_idx"][:, None], 1)[:, 0]
    loss = _mse_plus_hdr(pred, batch["rad"].to(pred.dtype), scene.max_i)
    assert cm.dtype == torch.float16 and loss.dtype == torch.float16
    loss.backward()
    torch.cuda.synchronize(dev)
    got = {"color_map_fine": cm, "color_map_atmo": atmo, "color_map_surf": surf}
    A, C, spread = shared["arms"]["A"], shared["arms"]["C"], shared["spread"]
    rec = {"loss": loss.item(), "loss_A": A["loss"].item(), "loss_C": C["loss"].item()}
    failures = []
    for k in MAPS:
        to_a = int(_f16_steps(got[k], A["res"][k]).max().item())
        to_c = int(_f16_steps(got[k], C["res"][k]).max().item())
        a_c = int(_f16_steps(A["res"][k], C["res"][k]).max().item())
        rec[k] = {"max_f16_steps_to_A": to_a, "max_f16_steps_to_C": to_c,
                  "max_f16_steps_A_to_C": a_c}
        if to_a > max(1, a_c):
            failures.append((k, rec[k]))
    for m in ref_ingp.MODULES:
        g = mods[m].params.grad.double().cpu()
        to_a, to_c = _rel(g, A["grad"][m]), _rel(g, C["grad"][m])
        c_a = _rel(C["grad"][m], A["grad"][m])
        bar = max(TOL["grad"], 4 * spread[m]) + c_a
        rec["grad_" + m] = {"rel_to_A": to_a, "rel_to_C": to_c, "rel_C_to_A": c_a, "bar": bar,
                            "x128_f16": bool(_f16_representable(mods[m].params.grad * LS).all())}
        if to_a > bar:
            failures.append((m, rec["grad_" + m]))
    _REC["bare_import_swap"] = rec
    _dump()
    print("bare import swap", rec)
    assert torch.equal(z_vals.cpu(), A["res"]["z_vals_fine"])
    assert not failures, (failures, rec)
