"""Shared pieces of the render tests and tools/render_timing.py (not collected by pytest):
the scaling that makes the composite alive, and the build-numerics composite error against
an f64 composite of the existing field forward's per-sample outputs."""

from __future__ import annotations

import torch

MAPS = ("color_map_fine", "color_map_atmo", "color_map_surf")
# hash-table factors tried in order, starting from the factor of the existing live tests
# (x 10 at N = 64, x 300 at N = 1,024). The seeded table is uniform in +-1e-4 and the
# networks have no bias, so sigma grows in proportion: a surface transmittance of 0.5 on the
# 16 x 16 scene's rays takes a factor of 3e3 to 1e4, an f16 alpha of 1 about 1e6.
LADDER = (1.0, 3.0, 10.0, 30.0, 100.0, 300.0, 1e3, 3e3, 1e4, 3e4, 1e5)


def base_factor(n_samples: int) -> float:
    return 10.0 if n_samples <= 128 else 300.0


def transmittance(res) -> torch.Tensor:
    """Per ray, the surface transmittance color_map_surf / color_surf at the band with the
    largest surface colour (NaN where the surface colour is zero in every band)."""
    cs = res["color_surf"].double()
    ms = res["color_map_surf"].double()
    best = cs.argmax(dim=1, keepdim=True)
    c = torch.take_along_dim(cs, best, 1)[:, 0]
    m = torch.take_along_dim(ms, best, 1)[:, 0]
    return torch.where(c > 0, m / c, torch.full_like(c, float("nan")))


def alive(res) -> tuple[bool, str]:
    """The precondition of every GPU case, on the EXISTING forward's outputs: at least a
    quarter of the rays have a surface transmittance below 0.5, at least one ray has it
    above 0, and color_map_atmo is nonzero."""
    t = transmittance(res)
    n = t.shape[0]
    below, above = int((t < 0.5).sum()), int((t > 0).sum())
    atmo = bool((res["color_map_atmo"] != 0).any())
    return (4 * below >= n and above >= 1 and atmo,
            f"{below}/{n} rays below 0.5, {above} above 0, atmo nonzero: {atmo}")


def make_alive(pipe, batch, u, extra=None):
    """Scale the position hash table up the ladder until forward's outputs meet the
    precondition (and ``extra(res)``, where given); returns (factor, forward results).
    Asserts that some factor does: a case that cannot is a bug of the test."""
    orig = pipe.pos_encoder.params.detach().clone()
    n = pipe.config["num_samples_per_ray"]
    said = []
    for step in LADDER:
        f = base_factor(n) * step
        with torch.no_grad():
            pipe.pos_encoder.params.copy_(orig * f)  # moves _version: the f16 copy refreshes
            res = pipe.forward(batch, u=u)
        ok, msg = alive(res)
        if ok and extra is not None:
            ok, more = extra(res)
            msg += "; " + more
        said.append(f"x{f:g}: {msg}")
        if ok:
            print(f"alive at table x{f:g}: {msg}")
            return f, res
    raise AssertionError("no table factor makes the composite alive: " + " | ".join(said))


def f64_maps(z_km, color, sigma, color_surf):
    """datasets.synthetic.render_surface_f64 (graphics_utils.py:6-77, f64) with a colour per
    sample and band: z_km (R, n), color (R, n, C), sigma (R, n), color_surf (R, C) ->
    (color_map, atmo, surf), each (R, C). render_surface_f64 itself takes one colour per ray;
    for such a colour the two agree exactly (checked where this is used)."""
    mid = (z_km[:, :-1] + z_km[:, 1:]) / 2
    mid = torch.cat([z_km[:, :1] * 0, mid, z_km[:, -1:]], dim=1)
    delta = torch.diff(mid, dim=1)
    alpha = 1 - torch.exp(-sigma * delta)
    ones = torch.ones_like(alpha[:, :1])
    weights = alpha * torch.cumprod(torch.cat([ones, 1 - alpha + 1e-10], dim=1), dim=1)[:, :-1]
    atmo = (color * weights[:, :, None]).sum(dim=1)
    surf = (1 - alpha).prod(dim=1)[:, None] * color_surf
    return atmo + surf, atmo, surf


def composite_errors(pipe, batch, u):
    """Build numerics: for each map, e = max |map - yardstick| / max |yardstick| of the fused
    render and of the existing forward, the yardstick being the f64 composite of the
    existing field forward's per-sample sigma and colour (all N samples: the field function
    called directly), with forward's z and color_surf. Returns {map: (e_render, e_forward)}."""
    from atmonr_amd.datasets.synthetic import render_surface_f64
    from atmonr_amd.field import IngpFieldFn
    from atmonr_amd.samplers import sample_and_preprocess

    B = batch["origin"].shape[0]
    N = pipe.config["num_samples_per_ray"]
    with torch.no_grad():
        fwd = pipe.forward(batch, u=u)
        _, z, coords = sample_and_preprocess(batch, N, pipe._prep_ngp, u=u)
        sigma, color = IngpFieldFn.apply(coords.view(B * N, 3), batch["dir"].float(), N,
                                         pipe.pos_encoder.params, pipe.pos_mlp.params,
                                         pipe.dir_mlp.params, pipe)
        ren = pipe.render(batch, u=u, fused=True)
    assert torch.equal(z, fwd["z_vals_fine"])
    # the field function's samples are forward's (results hold all but the last)
    assert torch.equal(sigma.view(B, N)[:, :-1], fwd["sigma_fine"][..., 0])
    assert torch.equal(color.view(B, N, -1)[:, :-1], fwd["color_fine"])
    z_km = z.double() * (float(pipe.scale) / 1000)
    sg, col = sigma.view(B, N).double(), color.view(B, N, -1).double()
    cs = fwd["color_surf"].double()
    yard = dict(zip(MAPS, f64_maps(z_km, col, sg, cs)))
    # f64_maps is render_surface_f64 where that function applies: one colour per ray
    flat = col[:, :1, 0].expand(B, N)
    want = render_surface_f64(z_km, flat[:, 0], sg, cs[:, 0])
    got = f64_maps(z_km, flat[:, :, None], sg, cs[:, :1])[0][:, 0]
    assert torch.allclose(got, want, rtol=1e-12, atol=0), (got - want).abs().max()
    out = {}
    for k in MAPS:
        top = yard[k].abs().max().item()
        assert top > 0, k
        out[k] = ((ren[k].double() - yard[k]).abs().max().item() / top,
                  (fwd[k].double() - yard[k]).abs().max().item() / top)
    return out
