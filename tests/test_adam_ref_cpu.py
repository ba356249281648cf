"""The K10 reference itself (tests/adam_ref.py), on the CPU.

The GPU tests (test_adam_exact_gpu.py) hold csrc/adam.hip to ``adam_step_f32`` bit for bit,
so this file shows that ``adam_step_f32`` is Adam:

* over 20 steps from zero state on workload-shaped inputs (tables in +-1e-4, sparse
  gradients spanning 1e-22..1e-2, eps = 1e-15), in AdamW wd 0, AdamW wd 1e-2 and Adam-L2
  wd 1e-3, its error against torch.optim in float64 is at most 4 times the error of
  torch.optim in float32 against the same, in p, exp_avg and exp_avg_sq. (Measured, seed 0,
  emulation / torch f32: max|dp| / (lr*steps) 1.6e-7 / 1.4e-7, 3.1e-7 / 2.7e-7 and
  1.6e-7 / 1.2e-7 for the three modes; exp_avg 9.2e-8 / 3.7e-8 of max|g| for AdamW and
  1.8e-7 / 1.3e-7 for Adam-L2; exp_avg_sq 1.3e-6 / 5.5e-7 relative for AdamW and
  1.9e-6 / 1.2e-6 for Adam-L2. The exp_avg_sq ratio is the kernel's ``1.0f - beta2`` from
  the f32 beta against torch's double ``1 - beta2``, a constant ~1.2e-6.) For Adam-L2 the
  scale of exp_avg is the largest |g + wd*p|, the gradient that reaches the moments: wd*p
  (~1e-7) dwarfs most g there, so max|g| is not exp_avg's scale;
* the regime exercises eps: dropping it, moving it inside the square root or using 1e-8
  changes the bits of at least 1 % of the elements;
* one f32 step from consistent states (steps 1, 5, 20 of the trajectory) stays within
  1 ulp (exp_avg) and 2 ulp (normal exp_avg_sq) of the float64 formula.
"""

import numpy as np
import pytest
import torch

from tests import adam_ref as ar

N, STEPS, FACTOR = 50_000, 20, 4.0
f32 = np.float32


@pytest.fixture(scope="module")
def inputs():
    rng = np.random.default_rng(0)
    return ar.workload_params(rng, N), ar.workload_grads(rng, N, STEPS)


def _chain(p0, grads, decoupled, wd, denom=None, keep=()):
    p, m, v = p0.copy(), np.zeros(len(p0), f32), np.zeros(len(p0), f32)
    states = {}
    for k, g in enumerate(grads):
        if k + 1 in keep:
            states[k + 1] = (p, m, v, g)
        p, m, v, _ = ar.adam_step_f32(p, g, m, v, wd=wd, decoupled=decoupled, step=k + 1,
                                      _denom=denom, **ar.HYPER)
    return (p, m, v), states


@pytest.fixture(scope="module")
def runs(inputs):
    """mode -> final emulated state and the states entering steps 1, 5, 20 (shared, read-only)."""
    p0, grads = inputs
    return {name: _chain(p0, grads, dec, wd, keep=(1, 5, 20)) for name, dec, wd in ar.MODES}


@pytest.mark.parametrize("name,decoupled,wd", ar.MODES)
def test_emulation_within_torch_f32_noise_of_torch_f64(inputs, runs, name, decoupled, wd):
    p0, grads = inputs
    ref64 = ar.torch_trajectory(p0, grads, decoupled=decoupled, wd=wd, dtype=torch.float64)
    t32 = ar.torch_trajectory(p0, grads, decoupled=decoupled, wd=wd, dtype=torch.float32)
    gmax = ar.moment_gradient_max(p0, grads, decoupled=decoupled, wd=wd)
    kw = dict(lr=ar.HYPER["lr"], steps=STEPS)
    emu = ar.trajectory_errors(runs[name][0], ref64, gmax, **kw)
    tor = ar.trajectory_errors(t32, ref64, gmax, **kw)
    print(f"{name}: emulation {emu}, torch f32 {tor}")
    # where no gradient ever reached the moments both moments are exact zeros
    off = gmax == 0
    assert not runs[name][0][1][off].any() and not runs[name][0][2][off].any()
    for k in emu:
        assert tor[k] > 0.0, k
        assert emu[k] <= FACTOR * tor[k], (name, k, emu[k], tor[k])


MUTATIONS = {
    "dropped": lambda v, bs, eps: np.sqrt(v) / bs,
    "inside_sqrt": lambda v, bs, eps: np.sqrt(v + eps) / bs,
    "1e-8": lambda v, bs, eps: np.sqrt(v) / bs + f32(1e-8),
}


@pytest.mark.parametrize("name,decoupled,wd", ar.MODES)
@pytest.mark.parametrize("mutation", list(MUTATIONS))
def test_regime_exercises_eps(inputs, runs, name, decoupled, wd, mutation):
    """A wrong eps changes the bits of >= 1 % of the elements after one step already, and
    at the end of the trajectory."""
    p0, grads = inputs
    one, _ = _chain(p0, grads[:1], decoupled, wd)
    one_mut, _ = _chain(p0, grads[:1], decoupled, wd, denom=MUTATIONS[mutation])
    end_mut, _ = _chain(p0, grads, decoupled, wd, denom=MUTATIONS[mutation])
    first = ar.bits_differ(one[0], one_mut[0]).mean()
    last = ar.bits_differ(runs[name][0][0], end_mut[0]).mean()
    print(f"{name} eps {mutation}: p differs in {first:.2%} after step 1, {last:.2%} after "
          f"step {STEPS}")
    assert first >= 0.01 and last >= 0.01


@pytest.mark.parametrize("name,decoupled,wd", ar.MODES)
@pytest.mark.parametrize("at", [1, 5, 20])
def test_one_f32_step_against_f64(runs, name, decoupled, wd, at):
    """exp_avg is a convex combination formed in three roundings: g - m within ulp(M) for
    M = max(|m_old|, |g|), scaled by w1 = 0.1, plus half an ulp each for the product and
    the sum: under 1 ulp(M). exp_avg_sq: 2 ulp where it is normal.

    With Adam's L2 term the gradient of the moments is g + wd*p, and here wd*p (~1e-7)
    dwarfs most g, with either sign: the f32 sum cancels, and no f32 evaluation stays
    within a few ulp of float64 in the moments (measured at step 1: exp_avg 87 ulp of
    max(|m_old|, |g + wd*p|), exp_avg_sq 1103 ulp). So in that mode the sum is held to its
    own bound -- one rounding of wd*p, one of the sum -- and both precisions then take the
    moments from the f32 sum, to the same 1 and 2 ulp."""
    p, m, v, g = runs[name][1][at]
    if not decoupled:
        wp = f32(wd) * p
        g, ge64 = g + wp, g.astype(np.float64) + float(f32(wd)) * p.astype(np.float64)
        bound = 0.5 * np.spacing(np.abs(wp)).astype(np.float64) + 0.5 * np.spacing(np.abs(g))
        assert (np.abs(g - ge64) <= bound).all()
        wd = 0.0
    kw = dict(wd=wd, decoupled=decoupled, step=at, **ar.HYPER)
    _, m32, v32, _ = ar.adam_step_f32(p, g, m, v, **kw)
    _, m64, v64, _, ge = ar.adam_step_f64(p, g, m, v, with_grad=True, **kw)
    scale = np.maximum(np.abs(m.astype(np.float64)), np.abs(ge)).astype(f32)
    em = np.abs(m32.astype(np.float64) - m64) / np.spacing(scale).astype(np.float64)
    normal = v64 >= float(np.finfo(f32).tiny)
    ev = (np.abs(v32.astype(np.float64) - v64)[normal]
          / np.spacing(v64.astype(f32))[normal].astype(np.float64))
    print(f"{name} step {at}: exp_avg {em.max():.3f} ulp, exp_avg_sq {ev.max():.3f} ulp "
          f"({int(normal.sum())} normal)")
    assert em.max() <= 1.0
    assert ev.max() <= 2.0


def test_edge_values_hold_what_they_claim():
    p, g, m, v = ar.edge_values(4099)
    with np.errstate(all="ignore"):
        sq = g * g
    tiny = float(np.finfo(f32).tiny)
    assert ((g == 0) & (m == 0) & (v == 0)).any() and ((g == 0) & (m != 0) & (v > 0)).any()
    assert ((g != 0) & (sq == 0)).any()                       # g*g underflows
    assert ((sq > 0) & (sq < tiny)).any()                      # g*g denormal
    near = np.sqrt(f32(0.01) * sq) / f32(0.1)                  # sqrt(v)/sqrt(bc2) at step 1
    assert ((near > 1e-16) & (near < 1e-14)).sum() > 10        # comparable with eps
    assert np.isinf(sq[np.isfinite(g)]).any()                  # g*g overflows
    assert np.isposinf(g).any() and np.isneginf(g).any() and np.isnan(g).any()
    for s in (128.0, 1000.0):                                  # both sides of the f16 overflow
        q = ar.quant_f16(g, s)
        fin = np.isfinite(g) & (np.abs(g) < 1e3)
        assert np.isinf(q[fin]).any()
        assert (np.isfinite(q[fin]) & (np.abs(g[fin]) > 60000.0 / s)).any()
    assert (np.signbit(g) & (g == 0)).any() and (np.signbit(p) & (p == 0)).any()
    assert ((v > 0) & (v < tiny)).any() and (v >= 0).all()
    for n in (0, 1, 255):
        assert all(len(x) == n and x.dtype == f32 for x in ar.edge_values(n, seed=3))


def test_adam_scalars_and_quantisation_follow_the_kernel():
    ss, bs, dec = ar.adam_scalars(1e-2, 0.9, 0.99, 1e-2, 1)
    b1, b2, lr = float(f32(0.9)), float(f32(0.99)), float(f32(1e-2))
    assert ss == f32(lr / (1.0 - b1)) and bs == f32((1.0 - b2) ** 0.5)
    assert dec == f32(1.0 - lr * float(f32(1e-2)))
    assert ar.adam_scalars(1e-2, 0.9, 0.99, 0.0, 50000) == (f32(1e-2), f32(1.0), f32(1.0))
    g = np.array([511.75, 511.9, -512.0, 3e-9, 1e-10, -0.0], f32)
    q = ar.quant_f16(g, 128.0)
    assert q[0] == 511.75 and np.isposinf(q[1]) and np.isneginf(q[2])
    assert q[3] == np.float16(np.float16(f32(3e-9) * f32(128)) * f32(1 / 128)) and q[4] == 0
    assert np.signbit(q[5]) and q[5] == 0
    a = np.array([np.nan, 1.0, -0.0], f32)
    b = np.array([-np.nan, 1.0, 0.0], f32)
    assert ar.bits_differ(a, b).tolist() == [False, False, True]
    with pytest.raises(AssertionError):
        ar.assert_bits_equal(a, b)
