"""tests/composite_oracle.py checked by itself, before any kernel is involved: the closed
form equals f64 autograd of the reference's formula, the reference's own f32 arithmetic
stays inside the error model, and the optically thick regimes really contain what they are
there for (samples behind an absorber that the bound still resolves, alpha == 1, T == 0)."""

import numpy as np
import pytest
import torch

from oracle import ref_path
from tests import composite_oracle as co


@pytest.mark.parametrize("S", [1, 4])
@pytest.mark.parametrize("N", [2, 65, 300])
def test_closed_form_equals_f64_autograd(N, S):
    """ref_path.render_with_surface on f64 tensors with z on a 2^-10 grid (the f32 delta is
    then exact), all five upstream gradients present, every output and gradient within a
    millionth of the model's bound.

    The reference forms alpha as 1 - exp(-x), which in f64 is an absolute 2^-53 or so off
    (and differs by that much between two exp implementations), while the oracle's
    -expm1(-x) is relatively exact: at x = 1e-5 that alone is 1.5e-6 of alpha's bound. So
    alpha is held to 2^-52 absolute, and the closed form is then evaluated on the reference's
    own alpha, where the two sides differ by f64 rounding only."""
    B = 7
    for regime in co.REGIMES:
        inp = co.make_inputs(regime, B, N, S, seed=11, z_grid=2.0 ** -10)
        ups = co.make_upstream(B, N, S, seed=11)
        z64 = inp["z"].astype(np.float64)
        mid = np.concatenate([z64[:, :1] * 0, (z64[:, :-1] + z64[:, 1:]) / 2, z64[:, -1:]], axis=1)
        assert np.array_equal(co.delta_f32(inp["z"], 1.0).astype(np.float64),
                              np.diff(mid, axis=1))
        t = {k: torch.from_numpy(inp[k].astype(np.float64)).requires_grad_(True)
             for k in ("z", "color", "sigma", "cs")}
        g = {k: torch.from_numpy(v.astype(np.float64)) for k, v in ups.items()}
        cm, alpha, w, atmo, surf = ref_path.render_with_surface(t["z"], t["color"], t["sigma"],
                                                                t["cs"])
        ((cm * g["d_cm"]).sum() + (alpha * g["d_alpha"]).sum() + (w * g["d_w"]).sum()
         + (atmo * g["d_atmo"]).sum() + (surf * g["d_surf"]).sum()).backward()
        got = {"cm": cm, "alpha": alpha, "w": w, "atmo": atmo, "surf": surf,
               "dcolor": t["color"].grad, "dsigma": t["sigma"].grad, "dcs": t["cs"].grad,
               "dz": t["z"].grad}
        got = {k: v.detach().numpy() for k, v in got.items()}
        own = co.evaluate(inp, ups, np.float64, model=True)
        assert np.abs(own["alpha"] - got["alpha"]).max() <= 2.0 ** -52
        ref = co.evaluate(inp, ups, np.float64, model=True, alpha=got["alpha"])
        direct = co.ratios(got, own)
        for k, r in co.ratios(got, ref).items():
            assert np.isfinite(got[k]).all(), (regime, k)
            print(f"{regime} N={N} S={S} {k}: {r.max():.3e} (on -expm1: {direct[k].max():.3e})")
            assert r.max() <= 1e-6, (regime, k, float(r.max()))


@pytest.mark.parametrize("S", [1, 4])
@pytest.mark.parametrize("N", co.LADDER)
def test_reference_f32_stays_inside_the_model(N, S):
    """With all five upstream gradients and with d_cm alone (the training loss)."""
    for regime in co.REGIMES:
        for which in (co.UPSTREAM, ("d_cm",)):
            _, _, ref, r32, rat = co.cell(regime, N, S, which=which)
            for k in co.QUANTITIES:
                assert np.isfinite(r32[k]).all() and np.isfinite(ref[k]).all(), (regime, k)
                print(f"{regime} N={N} S={S} {len(which)} upstream {k}: {rat[k].max():.3f}")
                assert rat[k].max() <= 1.0, (regime, which, k, float(rat[k].max()))


@pytest.mark.parametrize("S", [1, 4])
@pytest.mark.parametrize("N", [n for n in co.LADDER if n >= 63])
@pytest.mark.parametrize("regime", ["cloud", "wall"])
def test_thick_regimes_are_not_empty(regime, N, S):
    _, _, ref, r32, _ = co.cell(regime, N, S)
    thick = ref["t"] < 0.5
    behind = (np.cumsum(thick, axis=1) - thick) > 0          # some j < i has t_j < 0.5
    live = behind & (co.bounds(ref)["dsigma"] > 100 * co.FLOOR)
    print(f"{regime} N={N} S={S}: {live.mean():.3f} of dsigma behind an absorber and resolved")
    assert live.mean() >= 0.15
    assert (r32["alpha"] == 1.0).any()
    t32 = (np.float32(1) - r32["alpha"]) + np.float32(1e-10)
    T = np.ones_like(t32)
    T[:, 1:] = np.cumprod(t32[:, :-1], axis=1, dtype=np.float32)
    assert T.dtype == np.float32 and (T == 0.0).any()
