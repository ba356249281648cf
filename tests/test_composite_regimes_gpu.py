"""K8 (csrc/composite.hip) against the per-sample f64 oracle of tests/composite_oracle.py, in
four optical-depth regimes (thin air, optical depth ~3, a cloud slab, an alpha == 1 wall)
and on every kernel form: the register-blocked kernels at each samples-per-lane count with
one and four waves per ray, the generic kernels in the bands between them, partial last lanes
and waves at N = 64k +- 1, f32 and f16 storage, every null-pointer branch of the upstream
gradients and of the optional outputs.

Every output element must lie within 4 x max(1, r) of the oracle's bound, r being the ratio
the reference's own sequential f32 arithmetic reaches at that element: 4 covers tree-ordered
scans against sequential ones and a device expm1f / expf of up to 2 ulp against NumPy's.
ANR_COMPOSITE_REGIMES_OUT names a JSON file that receives, per (regime, N, S, path,
upstream set, quantity), the kernel's worst ratio beside the restatement's.

With d_surf as the only upstream gradient, dL/dalpha is the term r * prod_{k!=i}(1-alpha_k)
alone, whose f32 error comes from the factors behind sample i as well, while the model's A
counts those in front: there the restatement itself leaves the bound (6e4 in cloud at N = 65,
S = 4) and the kernel is held to the restatement, which it matches to seven digits.
"""

import contextlib
import json
import os

import numpy as np
import pytest
import torch

from tests import composite_oracle as co

pytestmark = pytest.mark.gpu

FACTOR = 4.0
ALL, CM_ONLY = co.UPSTREAM, ("d_cm",)
SINGLES = (("d_w",), ("d_alpha",), ("d_atmo",), ("d_surf",))
_record = {}


@pytest.fixture(scope="module", autouse=True)
def _write_record():
    yield
    out = os.environ.get("ANR_COMPOSITE_REGIMES_OUT")
    if out and _record:
        os.makedirs(os.path.dirname(out) or ".", exist_ok=True)
        keys = ("kind", "regime", "N", "S", "C", "path", "upstream", "quantity")
        with open(out, "w") as f:
            json.dump([dict(zip(keys, k), kernel=v[0], restatement=v[1])
                       for k, v in sorted(_record.items())], f, indent=1)


@contextlib.contextmanager
def dispatch(path):
    from atmonr_amd import _lib

    lib = _lib.load()
    prev = lib.anr_composite_force_generic(1 if path == "generic" else 0)
    try:
        yield
    finally:
        lib.anr_composite_force_generic(prev)


def _blocked(N, S, bwd, C=4):
    """launch_rb covers the shape: one wave per ray up to 256 samples, 4 waves up to 4096;
    the backward with 16 samples per lane and 4 density channels is left to the generic."""
    if C != 4 or N > 4096:
        return False
    return N <= 256 or ((N + 255) // 256 in (2, 3, 4, 8, 16)
                        and not (bwd and S == 4 and N > 3840))


def _bwd_refused(N, S, path, C=4):
    """The generic backward stages (2S+1)*N floats per ray in LDS, 64 KiB at the most."""
    generic = path == "generic" or not _blocked(N, S, True, C)
    return generic and (2 * S + 1) * N * 4 > 64 * 1024


def run(dev, inp, ups, f16=False, skip=(), bwd=True, buffers=None):
    """anr_composite_fwd and anr_composite_bwd on one cell; outputs start as NaN so that an
    element the kernel does not write is caught. ``skip``: outputs passed as null.
    ``buffers``: a dict that receives the device tensors before the backward is called."""
    from atmonr_amd import _lib

    dt = torch.float16 if f16 else torch.float32
    code = _lib.F16 if f16 else _lib.F32

    def tt(a):
        return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev).to(dt)

    z = torch.from_numpy(np.ascontiguousarray(inp["z"])).to(dev)
    color, sigma, cs = tt(inp["color"]), tt(inp["sigma"]), tt(inp["cs"])
    B, N, C = color.shape
    S = sigma.shape[2]

    def new(name, *shape, dtype=dt):
        if name in skip:
            return None
        return torch.full(shape, float("nan"), device=dev, dtype=dtype)

    o = {"cm": new("cm", B, C), "atmo": new("atmo", B, C), "surf": new("surf", B, C),
         "w": new("w", B, N, S), "alpha": new("alpha", B, N, S)}
    s, ptr = _lib.stream(dev), _lib.ptr
    zs = float(inp["z_scale"])
    _lib.call("anr_composite_fwd", ptr(z), zs, ptr(color), ptr(sigma), ptr(cs), code, B, N, C, S,
              ptr(o["cm"]), ptr(o["atmo"]), ptr(o["surf"]), ptr(o["w"]), ptr(o["alpha"]), s)
    if bwd:
        o.update({"dcolor": new("dcolor", B, N, C), "dsigma": new("dsigma", B, N, S),
                  "dcs": new("dcs", B, C), "dz": new("dz", B, N, dtype=torch.float32)})
        g = {k: tt(ups[k]) for k in co.UPSTREAM}
        if buffers is not None:
            buffers.update(o)
        _lib.call("anr_composite_bwd", ptr(z), zs, ptr(color), ptr(sigma), ptr(cs), code, B, N,
                  C, S, ptr(g["d_cm"]), ptr(g["d_atmo"]), ptr(g["d_surf"]), ptr(g["d_w"]),
                  ptr(g["d_alpha"]), ptr(o["dcolor"]), ptr(o["dsigma"]), ptr(o["dcs"]),
                  ptr(o["dz"]), s)
    torch.cuda.synchronize(dev)
    return {k: v.double().cpu().numpy() for k, v in o.items() if v is not None}


def check(got, cell, key, f16=False):
    """Finite, alpha in [0, 1], and elementwise within FACTOR * max(1, restatement)."""
    _, _, ref, r32, rr = cell
    if f16:
        rr = co.ratios(r32, ref, extra=co.f16_rounding)
    kr = co.ratios(got, ref, extra=co.f16_rounding if f16 else None)
    for q, k in kr.items():
        assert np.isfinite(got[q]).all(), (key, q, "not finite")
        rec = _record.setdefault(key + (q,), [0.0, 0.0])
        rec[0], rec[1] = max(rec[0], float(k.max())), max(rec[1], float(rr[q].max()))
        lim = FACTOR * np.maximum(1.0, rr[q])
        if not (k <= lim).all():
            i = np.unravel_index(np.argmax(k / lim), k.shape)
            pytest.fail(f"{key} {q}{list(i)}: kernel {got[q].reshape(k.shape)[i]!r} oracle "
                        f"{ref[q][i]!r} ratio {k[i]:.3g} (restatement {rr[q][i]:.3g})")
    if "alpha" in got:
        assert (got["alpha"] >= 0).all() and (got["alpha"] <= 1).all(), (key, "alpha range")


def _name(which):
    return "all" if which == ALL else "+".join(which)


def sweep(dev, kind, N, S, path, sets, regimes=co.REGIMES, C=4, **kw):
    f16 = kw.get("f16", False)
    with dispatch(path):
        for regime in regimes:
            for which in sets:
                cell = co.cell(regime, N, S, which=which, C=C, **kw)
                got = run(dev, cell[0], cell[1], f16=f16)
                check(got, cell, (kind, regime, N, S, C, path, _name(which)), f16=f16)


LADDER_CASES = [(N, S, p) for N in co.LADDER for S in (1, 4) for p in ("default", "generic")
                if not _bwd_refused(N, S, p)]
REFUSED_CASES = [(N, p) for N in (2048, 2049, 3841, 4096, 4097) for p in ("default", "generic")
                 if _bwd_refused(N, 4, p)]


@pytest.mark.parametrize("N,S,path", LADDER_CASES)
def test_ladder(dev, N, S, path):
    sets = (CM_ONLY, ALL) + (SINGLES if N in (65, 513) else ())
    sweep(dev, "f32", N, S, path, sets)


def test_ladder_leaves_out_only_the_refused():
    assert {(N, p) for N, p in REFUSED_CASES} == {
        (2049, "default"), (3841, "default"), (4096, "default"), (4097, "default"),
        (2048, "generic"), (2049, "generic"), (3841, "generic"), (4096, "generic"),
        (4097, "generic")}
    assert len(LADDER_CASES) == 4 * len(co.LADDER) - len(REFUSED_CASES)


@pytest.mark.parametrize("N,path", REFUSED_CASES)
def test_generic_backward_refuses_what_does_not_fit_lds(dev, N, path):
    """S = 4 on the generic backward above 64 KiB of LDS: an error before any launch (the
    gradient buffers keep their NaN fill); the forward at the same shape still works."""
    from atmonr_amd._lib import ANRError

    with dispatch(path):
        for regime in co.REGIMES:
            cell = co.cell(regime, N, 4, which=CM_ONLY)
            buffers = {}
            with pytest.raises(ANRError, match="too large"):
                run(dev, cell[0], cell[1], buffers=buffers)
            torch.cuda.synchronize(dev)
            for k in ("dcolor", "dsigma", "dcs", "dz"):
                assert torch.isnan(buffers[k]).all(), k
            got = run(dev, cell[0], cell[1], bwd=False)
            check(got, cell, ("f32", regime, N, 4, 4, path, "forward"))


@pytest.mark.parametrize("C,S", [(3, 1), (1, 1), (8, 8)])
@pytest.mark.parametrize("N", [65, 300])
def test_generic_only_shapes(dev, N, C, S):
    sweep(dev, "f32", N, S, "default", (CM_ONLY, ALL), regimes=("unit", "cloud"), C=C)


@pytest.mark.parametrize("path", ["default", "generic"])
@pytest.mark.parametrize("S", [1, 4])
@pytest.mark.parametrize("N", [64, 193, 1024])
def test_f16_storage(dev, N, S, path):
    sweep(dev, "f16", N, S, path, (CM_ONLY, ALL), f16=True)


@pytest.mark.parametrize("path", ["default", "generic"])
@pytest.mark.parametrize("S", [1, 4])
@pytest.mark.parametrize("N", [65, 257, 1025])
def test_ties_zero_start_and_z_scale(dev, N, S, path):
    assert (co.delta_f32(co.cell("unit", N, S, ties=True)[0]["z"], co.Z_SCALE_VARIANT) == 0).any()
    sweep(dev, "ties", N, S, path, (CM_ONLY, ALL), ties=True)


SHAPES_PER_PATH = [(193, 1, "default"), (513, 4, "default"), (300, 4, "generic")]


@pytest.mark.parametrize("N,S,path", SHAPES_PER_PATH)
def test_optional_outputs(dev, N, S, path):
    """A null output pointer only drops that store: everything else keeps its bits."""
    cell = co.cell("cloud", N, S)
    with dispatch(path):
        full = run(dev, cell[0], cell[1])
        check(full, cell, ("f32", "cloud", N, S, 4, path, "all"))
        for name in ("w", "alpha", "atmo", "surf", "dz"):
            got = run(dev, cell[0], cell[1], skip=(name,))
            assert set(got) == set(full) - {name}
            for k, v in got.items():
                assert np.array_equal(v, full[k]), (name, k)


@pytest.mark.parametrize("N,S,path", SHAPES_PER_PATH)
def test_rays_are_independent(dev, N, S, path):
    """Permuting the rays permutes every output bit for bit."""
    inp, ups = co.cell("cloud", N, S)[:2]
    perm = np.random.default_rng(N).permutation(inp["z"].shape[0])
    pinp = {k: (v if k == "z_scale" else v[perm]) for k, v in inp.items()}
    pups = {k: v[perm] for k, v in ups.items()}
    with dispatch(path):
        a, b = run(dev, inp, ups), run(dev, pinp, pups)
    for k in a:
        assert np.array_equal(a[k][perm], b[k]), k
