"""A scalar-order reference of the K10 update (csrc/adam.hip) for the Adam tests: helpers, no tests.

``adam_step_f32`` performs one IEEE f32 operation per operation of the kernel, in the
kernel's order, with nothing fused (adam.hip is built with ``fp contract(off)`` and f32
denormals on), so a kernel output is compared with it bit for bit. ``adam_step_f64`` is the
same formula in float64 on the same f32 inputs and f32 scalars. torch's own optimizers are
no bit-level reference: they form ``1 - beta`` in double where the kernel forms
``1.0f - beta`` from the f32 betas that cross the ABI (exp_avg_sq offset by a constant
~1.2e-6 relative), and differ from the op-by-op order; ``torch_trajectory`` and
``trajectory_errors`` tie the two together by a tolerance that is torch-f32's own error
against torch-f64.
"""

from __future__ import annotations

import math

import numpy as np

f32 = np.float32

# lr, betas, eps of configs/instant_ngp.json; (name, decoupled, weight_decay)
HYPER = dict(lr=1e-2, b1=0.9, b2=0.99, eps=1e-15)
MODES = [("adamw_wd0", True, 0.0), ("adamw_wd1e-2", True, 1e-2), ("adam_l2_wd1e-3", False, 1e-3)]


def adam_scalars(lr, b1, b2, wd, step):
    """adam.hip's adam_scalars: every input at its f32 value, the arithmetic in double
    (Python's float ** is C's pow, as std::pow there), each result rounded to f32 once.
    Returns (step_size, bc2_sqrt, decay)."""
    lr, b1, b2, wd = (float(f32(x)) for x in (lr, b1, b2, wd))
    bc1 = 1.0 - b1 ** float(step)
    bc2 = 1.0 - b2 ** float(step)
    return f32(lr / bc1), f32(math.sqrt(bc2)), f32(1.0 - lr * wd)


def quant_f16(g, s):
    """adam.hip's quant_f16 (anr_grad_quantize_f16's rounding): f16(g*s), then
    f16(h1 * (1.0f/s)), the products in f32."""
    s = f32(s)
    with np.errstate(all="ignore"):
        h1 = (g * s).astype(np.float16).astype(f32)
        return (h1 * (f32(1.0) / s)).astype(np.float16).astype(f32)


def _denom_kernel(v, bc2_sqrt, eps):
    return np.sqrt(v) / bc2_sqrt + eps


def _step(ft, p, g, m, v, lr, b1, b2, eps, wd, decoupled, step, grad_quant, scalars, denom):
    if scalars is None:
        scalars = adam_scalars(lr, b1, b2, wd, step)
    step_size, bc2_sqrt, decay = scalars
    # the f32 values that cross the ABI, then the working precision
    b1, b2, eps, wd = (ft(f32(x)) for x in (b1, b2, eps, wd))
    step_size, bc2_sqrt, decay = ft(f32(step_size)), ft(f32(bc2_sqrt)), ft(f32(decay))
    one = ft(1.0)
    w1 = one - b1  # exact in f32 for 0.5 <= b1 < 1 (Sterbenz), so the same value in f64
    p, g, m, v = (np.asarray(x, dtype=f32) for x in (p, g, m, v))
    with np.errstate(all="ignore"):
        if grad_quant:
            g = quant_f16(g, grad_quant)  # a rounding specification: f32 products in both
        p, g, m, v = (x.astype(ft) for x in (p, g, m, v))
        if wd != 0:
            if decoupled:
                p = p * decay
            else:
                g = g + wd * p
        if w1 < ft(0.5):
            m = m + w1 * (g - m)
        else:
            m = g - (g - m) * (one - w1)
        v = v * b2 + (one - b2) * g * g
        p = p + (-step_size) * (m / (denom or _denom_kernel)(v, bc2_sqrt, eps))
    return p, m, v, g


def adam_step_f32(p, g, m, v, *, lr, b1, b2, eps, wd, decoupled, step, grad_quant=0.0,
                  scalars=None, _denom=None):
    """One update as adam.hip computes it: (p, m, v, p16), f32 / f32 / f32 / f16.
    ``scalars``: (step_size, bc2_sqrt, decay) to use instead of adam_scalars (the device-step
    form's own). ``_denom(v, bc2_sqrt, eps)``: a seam for the mutation guard of the CPU
    test, nothing else uses it."""
    p, m, v, _ = _step(f32, p, g, m, v, lr, b1, b2, eps, wd, decoupled, step, grad_quant,
                       scalars, _denom)
    assert p.dtype == m.dtype == v.dtype == f32
    with np.errstate(all="ignore"):
        return p, m, v, p.astype(np.float16)


def adam_step_f64(p, g, m, v, *, lr, b1, b2, eps, wd, decoupled, step, grad_quant=0.0,
                  scalars=None, with_grad=False):
    """The same formula in float64 on the same f32 inputs and f32 scalars: (p, m, v, p16).
    ``with_grad``: also the gradient that reached the moments (quantised, L2 term added)."""
    p, m, v, g = _step(np.float64, p, g, m, v, lr, b1, b2, eps, wd, decoupled, step,
                       grad_quant, scalars, None)
    with np.errstate(all="ignore"):
        out = (p, m, v, p.astype(np.float16))
    return out + (g,) if with_grad else out


def workload_grads(rng, n, steps):
    """[steps, n] f32 gradients of the shape the hash tables see: a fixed per-element scale,
    log-uniform over 1e-22..1e-2, a normal amplitude drawn at each step, and 70 % exact
    zeros at each step under a fresh mask."""
    scale = 10.0 ** rng.uniform(-22.0, -2.0, n)
    out = np.empty((steps, n), f32)
    for k in range(steps):
        g = (scale * rng.standard_normal(n)).astype(f32)
        g[rng.random(n) < 0.7] = 0.0
        out[k] = g
    return out


def workload_params(rng, n):
    """tcnn's table initialisation: uniform in +-1e-4."""
    return ((rng.random(n) * 2.0 - 1.0) * 1e-4).astype(f32)


def _logu(rng, lo, hi, n):
    return (10.0 ** rng.uniform(math.log10(lo), math.log10(hi), n)
            * rng.choice([-1.0, 1.0], n)).astype(f32)


def edge_values(n, seed=0):
    """One tensor (p, g, m, v; f32) of n elements in eight contiguous blocks:

    0  g = 0, zero state
    1  g = 0, non-zero state (coasting momentum)
    2  |g| log-uniform in 1e-24..1e-2: g*g underflows below ~4e-23, is denormal up to
       ~1e-19, and sqrt(v) ~ eps = 1e-15 around |g| ~ 1e-14; state zero on the even
       elements, of the gradient's own magnitude on the odd ones
    3  |g| log-uniform in 1e18..3e38: g*g overflows, v = inf, the update is 0
    4  g = +inf, -inf, NaN in turn
    5  g across the f16 overflow at loss scale 128 (|g|*128 around 65504..65520) and at
       loss scale 1000, the exact thresholds and their f32 neighbours included
    6  g = -0.0 with p, m = +-0.0 and zero / non-zero state
    7  denormal and near-denormal state under small g
    """
    rng = np.random.default_rng(1000 + seed)
    p = workload_params(rng, n)
    g = np.zeros(n, f32)
    m = np.zeros(n, f32)
    v = np.zeros(n, f32)
    blocks = [np.arange(n)[(np.arange(n) * 8) // max(n, 1) == b] for b in range(8)]

    def state(idx, mag):
        m[idx] = (mag * rng.standard_normal(len(idx))).astype(f32)
        with np.errstate(all="ignore"):
            sq = np.abs(mag).astype(np.float64) ** 2
            v[idx] = (sq * rng.uniform(0.1, 2.0, len(idx))).astype(f32)

    i = blocks[1]
    state(i, np.abs(_logu(rng, 1e-20, 1e-2, len(i))))
    i = blocks[2]
    g[i] = _logu(rng, 1e-24, 1e-2, len(i))
    state(i[1::2], np.abs(g[i[1::2]]))
    i = blocks[3]
    g[i] = _logu(rng, 1e18, 3e38, len(i))
    state(i[1::2], np.abs(_logu(rng, 1e-6, 1e-2, len(i[1::2]))))
    i = blocks[4]
    g[i] = np.resize(np.array([np.inf, -np.inf, np.nan], f32), len(i))
    state(i[3::6], np.full(len(i[3::6]), 1e-3, f32))
    i = blocks[5]
    thr = []
    for s in (128.0, 1000.0):
        for top in (65504.0, 65519.0, 65520.0, 65536.0):
            x = f32(top / s)
            thr += [x, np.nextafter(x, f32(0)), np.nextafter(x, f32(np.inf))]
    thr = np.array(thr + [-t for t in thr], f32)
    fill = np.concatenate([rng.uniform(400.0, 700.0, len(i)), rng.uniform(50.0, 80.0, len(i))])
    fill = (fill * rng.choice([-1.0, 1.0], len(fill))).astype(f32)
    g[i] = np.concatenate([thr, rng.permutation(fill)])[:len(i)]
    state(i[1::2], np.full(len(i[1::2]), 1e-3, f32))
    i = blocks[6]
    g[i] = -0.0
    p[i[0::4]] = -0.0
    p[i[1::4]] = 0.0
    m[i[0::2]] = -0.0
    state(i[3::4], np.full(len(i[3::4]), 1e-8, f32))
    m[i[3::8]] = -0.0
    i = blocks[7]
    g[i] = _logu(rng, 1e-30, 1e-18, len(i))
    m[i] = _logu(rng, 1e-44, 1e-36, len(i))
    v[i] = np.abs(_logu(rng, 1e-45, 1e-37, len(i)))
    return p, g, m, v


def _bits(x):
    x = np.ascontiguousarray(x)
    return x.view({2: np.uint16, 4: np.uint32, 8: np.uint64}[x.dtype.itemsize])


def bits_differ(a, b):
    """Boolean mask of the elements whose bit patterns differ, any NaN equal to any NaN
    (a NaN against a number differs)."""
    a, b = np.asarray(a), np.asarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape, (a.dtype, b.dtype, a.shape, b.shape)
    if a.dtype.kind == "f":
        na, nb = np.isnan(a), np.isnan(b)
        return (na != nb) | (~na & (_bits(a) != _bits(b)))
    return a != b


def assert_bits_equal(got, want, what=""):
    """Equal bit patterns element by element; any NaN equals any NaN and the NaN masks are
    equal."""
    d = bits_differ(got, want)
    if d.any():
        idx = np.flatnonzero(d)
        show = ", ".join(f"[{i}] {got.flat[i]!r} != {want.flat[i]!r}" for i in idx[:6])
        raise AssertionError(f"{what}: {len(idx)} of {d.size} elements differ in their bits: "
                             f"{show}")


def ulp_distance(a, b):
    """|a - b| in units of the f32 spacing at max(|a|, |b|) (finite inputs)."""
    a, b = np.asarray(a, f32), np.asarray(b, f32)
    sp = np.spacing(np.maximum(np.abs(a), np.abs(b))).astype(np.float64)
    return np.abs(a.astype(np.float64) - b.astype(np.float64)) / sp


def torch_trajectory(p0, grads, *, decoupled, wd, dtype, lr=HYPER["lr"], b1=HYPER["b1"],
                     b2=HYPER["b2"], eps=HYPER["eps"]):
    """torch.optim.AdamW / Adam (foreach=False) on the CPU in ``dtype`` from zero state over
    ``grads``: (p, exp_avg, exp_avg_sq) as float64 arrays."""
    import torch

    p = torch.nn.Parameter(torch.from_numpy(np.array(p0, f32)).to(dtype))
    opt = (torch.optim.AdamW if decoupled else torch.optim.Adam)(
        [p], lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd, foreach=False)
    for g in grads:
        p.grad = torch.from_numpy(np.array(g, f32)).to(dtype)
        opt.step()
    st = opt.state[p]
    return tuple(x.detach().double().numpy() for x in (p, st["exp_avg"], st["exp_avg_sq"]))


def moment_gradient_max(p0, grads, *, decoupled, wd, **hyper):
    """Per element, the largest |gradient that reached the moments| over the run, from a
    float64 run of the formula: max |g| for AdamW, max |g + wd*p| for Adam with L2 (there
    exp_avg follows wd*p wherever g itself is tiny, so |g| alone is not its scale)."""
    hp = {**HYPER, **hyper}
    p, m, v = np.array(p0, f32), np.zeros(len(p0), f32), np.zeros(len(p0), f32)
    gmax = np.zeros(len(p0))
    for k, g in enumerate(grads):
        p64, m64, v64, _, ge = adam_step_f64(p, g, m, v, wd=wd, decoupled=decoupled, step=k + 1,
                                             with_grad=True, **hp)
        gmax = np.maximum(gmax, np.abs(ge))
        p, m, v = p64.astype(f32), m64.astype(f32), v64.astype(f32)
    return gmax


def trajectory_errors(got, ref64, gmax, *, lr, steps):
    """The three error measures of a final (p, exp_avg, exp_avg_sq) against torch-f64's:
    max |dp| / (lr*steps); max |d exp_avg| / gmax where gmax > 0; the largest relative
    error of exp_avg_sq where the reference exceeds 1e-30."""
    p, m, v = (np.asarray(x, np.float64) for x in got)
    pr, mr, vr = ref64
    on = gmax > 0
    big = vr > 1e-30
    return {"p": float(np.max(np.abs(p - pr)) / (lr * steps)),
            "exp_avg": float(np.max(np.abs(m - mr)[on] / gmax[on])),
            "exp_avg_sq": float(np.max(np.abs(v - vr)[big] / vr[big]))}
