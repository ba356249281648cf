"""Per-sample f64 oracle, error model and inputs for the f32 composite (csrc/composite.hip).

NumPy only. ``evaluate`` is the closed form of render_with_surface (graphics_utils.py:6-77)
and of its autograd, O(N) per ray with sequential recurrences vectorised over the rays:

    x = sigma*delta   alpha = -expm1(-x)   e = exp(-x)   t = (1-alpha) + 1e-10
    T_i = prod_{j<i} t_j      w = alpha*T      atmo = sum_i w_i c_i
    surf = prod_i (1-alpha_i) * c_surf          cm = atmo + surf
    ga = d_cm + d_atmo        gs = d_cm + d_surf
    q_i = sum_c c_ic ga_c + d_w_i   (S == C: the term c == s only)     r likewise from c_surf, gs
    V_i = q_i alpha_i + t_i V_{i+1},  V_N = 0
    dalpha_i = T_i (q_i - V_{i+1}) - r prod_{k!=i}(1-alpha_k) + d_alpha_i   (prefix * suffix)
    dsigma = dalpha e delta     ddelta = sum_s dalpha e sigma     dcolor_ic = w_i ga_c
    dcsurf = prod(1-alpha) gs   dz = z_scale * (mid/diff map)^T ddelta

``delta`` is always formed in f32 in the reference's operation order (``delta_f32``) and only
then widened: the kernels are built with contraction off and keep that order, so delta is a
shared input. Formed in f64 it differs from any f32 evaluation by ulp(z)/delta (1e-4 relative
at 1,024 samples over 22.7 km), which would swamp every other error.

``evaluate(..., np.float32)`` is the same text run in f32 with sequential scans: the
reference-side yardstick a kernel is measured against.

Error model (``bounds``), eps = 2^-24, for every output element:

    bound = eps * scale * (8 + 2 A + 2 x + N_COEFF N) + 2^-120

``scale`` is the value's recurrence with every signed term replaced by its magnitude
(|value| where the value is one product); A = sum_{j<i} 1/t_j for a per-sample quantity and
sum_j 1/(1-alpha_j) for surf and dcsurf, because (1-alpha) carries an absolute error of an f32
ulp of 1; x = |x_i| is exp's conditioning (0 for per-ray quantities); N is the scan length;
2^-120 is the denormal floor. A is 0 for atmo, alpha and cm. ddelta sums its channels' terms,
each with its own A and x, and dz carries them through the mid/diff map with absolute
coefficients. ``ratios`` is |got - oracle| / bound, elementwise.
"""

from __future__ import annotations

import functools

import numpy as np

EPS = 2.0 ** -24
FLOOR = 2.0 ** -120
# Coefficient of N in the error model. 1 holds the sequential f32 restatement in every cell
# of the ladder but one: (unit, N=1, S=4, B=7), where cm = w c + (1-alpha) c_surf with alpha
# near 1 and a small c inherits the absolute error eps*c_surf of (1-alpha) while the model
# gives cm no A term; the restatement reaches 1.33 of the bound there. 8 + 4N = 12 at N = 1
# covers it (1.33 * 9 = 11.9).
N_COEFF = 4.0
Z_MAX = 22.7
Z_SCALE_VARIANT = 37.17
REGIMES = ("thin", "unit", "cloud", "wall")
QUANTITIES = ("cm", "atmo", "surf", "alpha", "w", "dcolor", "dsigma", "dcs", "dz")
UPSTREAM = ("d_cm", "d_atmo", "d_surf", "d_w", "d_alpha")
LADDER = (1, 2, 63, 64, 65, 128, 129, 192, 193, 256, 257, 512, 513, 768, 769, 1024, 1025, 1793,
          2048, 2049, 3841, 4096, 4097)


# ------------------------------------------------------------------------------- inputs
def _f32(a):
    return np.asarray(a, dtype=np.float32)


def make_inputs(regime, B, N, S, seed, C=4, z_grid=None):
    """{z (B,N), z_scale, color (B,N,C), sigma (B,N,S), cs (B,C)}, every value an f32.
    ``z_grid``: round z to multiples of it (2^-10 makes the f32 delta exact)."""
    assert regime in REGIMES and S in (1, C)
    rng = np.random.default_rng([seed, REGIMES.index(regime), N, S, C])
    z = np.sort(rng.uniform(0.0, Z_MAX, (B, N)), axis=1)
    if z_grid:
        z = np.round(z / z_grid) * z_grid
    color = rng.uniform(0.0, 2.0, (B, N, C))
    cs = rng.uniform(0.0, 2.0, (B, C))
    d = Z_MAX / N
    sigma = rng.uniform(1e-5, 2.1e-4, (B, N, S))
    if regime == "unit":
        sigma = rng.uniform(0.0, 6.0 / Z_MAX, (B, N, S))
    elif regime == "cloud":
        lens = (1, 2, 5, 17, 40, N // 4, N // 2)
        for b in range(B):
            i0 = min(N - 1, N // 3 + b)
            n = max(1, min(lens[b % 7], N - i0))
            sigma[b, i0:i0 + n] = rng.uniform(0.3, 8.3, (n, S)) / d
    elif regime == "wall":
        for b in range(B):
            i0 = min(N - 1, N // 2 + b)
            sigma[b, i0:i0 + b + 1] = 40.0 / d
    return {"z": _f32(z), "z_scale": 1.0, "color": _f32(color), "sigma": _f32(sigma),
            "cs": _f32(cs)}


def make_upstream(B, N, S, seed, C=4, which=UPSTREAM):
    """Signed upstream gradients in (-1, 1) for the names in ``which``; the others None."""
    rng = np.random.default_rng([seed, 77, N, S, C])
    shapes = {"d_cm": (B, C), "d_atmo": (B, C), "d_surf": (B, C), "d_w": (B, N, S),
              "d_alpha": (B, N, S)}
    full = {k: _f32(rng.uniform(-1.0, 1.0, shapes[k])) for k in UPSTREAM}
    return {k: (full[k] if k in which else None) for k in UPSTREAM}


def with_ties(inp, seed):
    """The same case with z_0 == 0, interior ties in z (delta == 0 there) and
    z_scale = 37.17 (the workload passes scale/1000); sigma is divided by the scale so that
    the optical depths stay those of the regime."""
    rng = np.random.default_rng([seed, 99])
    z = inp["z"].copy()
    B, N = z.shape
    z[:, 0] = 0.0
    for b in range(B):
        for i in rng.integers(1, max(2, N - 2), size=max(1, N // 16)):
            if i + 2 < N:  # three equal z: delta_{i+1} == 0 exactly
                z[b, i + 1] = z[b, i]
                z[b, i + 2] = z[b, i]
    zs = np.float32(Z_SCALE_VARIANT)
    out = dict(inp)
    out["z"] = z
    out["z_scale"] = float(zs)
    out["sigma"] = _f32(inp["sigma"] / zs)
    return out


def to_f16(inp, ups):
    """Inputs and upstream gradients rounded to f16 storage (z stays f32), as f32 arrays."""
    r = lambda a: None if a is None else a.astype(np.float16).astype(np.float32)  # noqa: E731
    inp = dict(inp, color=r(inp["color"]), sigma=r(inp["sigma"]), cs=r(inp["cs"]))
    return inp, {k: r(v) for k, v in ups.items()}


# --------------------------------------------------------------------------- evaluation
def delta_f32(z, z_scale):
    """graphics_utils.py:30-34 in f32: zs = z*z_scale, mid = [zs_0*0, (zs_i+zs_{i+1})/2 ...,
    zs_{N-1}], delta = diff(mid)."""
    zs = _f32(z) * np.float32(z_scale)
    mid = np.concatenate([zs[:, :1] * np.float32(0), (zs[:, :-1] + zs[:, 1:]) / np.float32(2),
                          zs[:, -1:]], axis=1)
    return np.diff(mid, axis=1)


def _excl_cumprod(a):
    out = np.ones_like(a)
    out[:, 1:] = np.cumprod(a[:, :-1], axis=1, dtype=a.dtype)
    return out


def _excl_rev_cumprod(a):
    return _excl_cumprod(a[:, ::-1])[:, ::-1]


def _seq_sum(a):
    """Sum over axis 1 in order (np.sum adds pairwise)."""
    return np.cumsum(a, axis=1, dtype=a.dtype)[:, -1]


def _suffix_affine(b, t):
    """V_i = b_i + t_i V_{i+1}, V_N = 0, along axis 1 of t (b may carry leading axes).
    Returns V_{i+1} for every i."""
    nxt = np.zeros_like(b)
    v = np.zeros_like(b[..., 0, :])
    for i in range(b.shape[-2] - 1, -1, -1):
        nxt[..., i, :] = v
        v = b[..., i, :] + t[:, i, :] * v
    return nxt


def _dz_map(dd, z_scale, absolute):
    """Transpose of the mid/diff map: dmid_j = dd_{j-1} - dd_j, then mid_j = (zs_{j-1} +
    zs_j)/2 for 1 <= j <= N-1, mid_0 = zs_0*0, mid_N = zs_{N-1}; times z_scale."""
    B, N = dd.shape
    sgn = 1.0 if absolute else -1.0
    dmid = np.zeros((B, N + 1), dtype=dd.dtype)
    dmid[:, 1:] += dd
    dmid[:, :N] += dd.dtype.type(sgn) * dd
    half = dd.dtype.type(0.5)
    dzs = np.zeros_like(dd)
    dzs[:, 1:] += half * dmid[:, 1:N]        # k >= 1: mid_k
    dzs[:, :N - 1] += half * dmid[:, 1:N]    # k + 1 <= N - 1: mid_{k+1}
    dzs[:, N - 1] += dmid[:, N]
    zs = dd.dtype.type(abs(z_scale) if absolute else z_scale)
    return dzs * zs


def evaluate(inp, ups, ft=np.float64, model=False, alpha=None):
    """Every output and gradient in precision ``ft`` from the f32 delta. ``ups``: upstream
    gradients by name, any of them None. With ``model`` also the error-model weight
    scale * (8 + 2A + 2x + N_COEFF N) of every quantity, under "m_<name>". ``alpha``: use
    these values instead of -expm1(-x) (the reference's 1 - exp(-x) cancels for small x and
    is an absolute 2^-53 or so off, far above a relative f64 rounding of alpha)."""
    ft = np.dtype(ft).type
    c = inp["color"].astype(ft)
    sg = inp["sigma"].astype(ft)
    cs = inp["cs"].astype(ft)
    B, N, C = c.shape
    S = sg.shape[2]
    one = ft(1)
    with np.errstate(under="ignore", over="ignore"):
        dl = delta_f32(inp["z"], inp["z_scale"]).astype(ft)[:, :, None]
        x = sg * dl
        e = np.exp(-x)
        alpha = -np.expm1(-x) if alpha is None else np.asarray(alpha, ft).reshape(x.shape)
        om = one - alpha
        t = om + ft(1e-10)
        T = _excl_cumprod(t)
        w = alpha * T
        wc = w if S == C else np.broadcast_to(w, (B, N, C))
        atmo = _seq_sum(c * wc)
        Pp = _excl_cumprod(om)
        Ptot = Pp[:, -1] * om[:, -1]                         # (B, S)
        surf = Ptot * cs
        out = {"alpha": alpha, "w": w, "atmo": atmo, "surf": surf, "cm": atmo + surf}

        def up(k, shape):
            return np.zeros(shape, ft) if ups.get(k) is None else ups[k].astype(ft)

        dcm = up("d_cm", (B, C))
        ga = dcm + up("d_atmo", (B, C))
        gs = dcm + up("d_surf", (B, C))
        dw, dal_up = up("d_w", (B, N, S)), up("d_alpha", (B, N, S))

        def chan(per_c):  # sum over c in order for S == 1, the term c == s for S == C
            if S == C:
                return per_c
            acc = np.zeros(per_c.shape[:-1] + (1,), ft)
            for k in range(C):
                acc = acc + per_c[..., k:k + 1]
            return acc

        q = chan(c * ga[:, None, :]) + dw
        r = chan(cs * gs)                                    # (B, S)
        terms = [q * alpha]
        if model:
            qa = chan(np.abs(c) * np.abs(ga)[:, None, :]) + np.abs(dw)
            terms.append(qa * alpha)
        Vn = _suffix_affine(np.stack(terms), t)
        pne = Pp * _excl_rev_cumprod(om)
        dalpha = T * (q - Vn[0]) - r[:, None, :] * pne + dal_up
        out["dsigma"] = dalpha * e * dl
        dd = _seq_sum(np.swapaxes(dalpha * e * sg, 1, 2))    # (B, N)
        out["dz"] = _dz_map(dd, inp["z_scale"], False)
        out["dcolor"] = wc * ga[:, None, :]
        out["dcs"] = Ptot * gs
        if not model:
            return out
        s_dal = T * (qa + Vn[1]) + np.abs(r)[:, None, :] * pne + np.abs(dal_up)
        A = np.cumsum(one / t, axis=1) - one / t             # sum_{j<i} 1/t_j
        As = np.sum(one / np.maximum(om, 1e-300), axis=1)    # (B, S)
        nn = 8.0 + N_COEFF * N
        per = nn + 2.0 * A + 2.0 * np.abs(x)                 # (B, N, S)
        perc = per if S == C else np.broadcast_to(per, (B, N, C))
        ray = nn + 2.0 * As                                  # (B, S)
        s_atmo = _seq_sum(np.abs(c) * wc)
        out["m_alpha"] = np.abs(alpha) * (nn + 2.0 * np.abs(x))
        out["m_w"] = np.abs(w) * per
        out["m_atmo"] = s_atmo * nn
        out["m_surf"] = np.abs(surf) * ray
        out["m_cm"] = (s_atmo + np.abs(surf)) * nn
        out["m_dcolor"] = np.abs(out["dcolor"]) * perc
        out["m_dcs"] = np.abs(out["dcs"]) * ray
        out["m_dsigma"] = s_dal * e * np.abs(dl) * per
        out["m_dz"] = _dz_map(np.sum(s_dal * e * np.abs(sg) * per, axis=2), inp["z_scale"], True)
        out["t"] = t
        return out


def bounds(ref):
    """name -> bound from an ``evaluate(..., model=True)`` result."""
    return {k: EPS * ref["m_" + k] + FLOOR for k in QUANTITIES}


def ratios(got, ref, extra=None):
    """name -> |got - oracle| / bound, elementwise, for the quantities present in ``got``.
    ``extra(name, oracle)`` adds to the bound (storage rounding)."""
    bd = bounds(ref)
    out = {}
    for k in QUANTITIES:
        if k in got:
            b = bd[k] + (extra(k, ref[k]) if extra else 0.0)
            out[k] = np.abs(np.asarray(got[k], np.float64).reshape(ref[k].shape) - ref[k]) / b
    return out


@functools.lru_cache(maxsize=16)
def cell(regime, N, S, which=UPSTREAM, C=4, B=7, ties=False, f16=False, seed=2024):
    """One cell of the test grid, computed once and shared (treat it as read-only):
    (inputs, upstream, f64 oracle with model, f32 restatement, the restatement's ratios)."""
    inp = make_inputs(regime, B, N, S, seed, C=C)
    ups = make_upstream(B, N, S, seed, C=C, which=which)
    if ties:
        inp = with_ties(inp, seed)
    if f16:
        inp, ups = to_f16(inp, ups)
    ref = evaluate(inp, ups, np.float64, model=True)
    r32 = evaluate(inp, ups, np.float32)
    return inp, ups, ref, r32, ratios(r32, ref)


def f16_rounding(name, oracle):
    """Output rounding of f16 storage (dz is always f32)."""
    return 0.0 if name == "dz" else 2.0 ** -11 * np.abs(oracle) + 2.0 ** -25
