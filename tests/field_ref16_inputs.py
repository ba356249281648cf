"""Seeded inputs and the oracle run of the reference-numerics field backward tests
(tests/test_field_ref16_oracle_cpu.py, tests/test_field_ref16_oracle_gpu.py). Everything
here runs on the CPU; the GPU test copies the tensors to the device.

The inputs follow test_ingp_field_bwd_ref16_rows_equals_f32_rows: enc uniform in [-1, 1]
as f16, weights randn * sqrt(2 / fan_in), dL/dcolor = randn * 1e-2 and dL/dsigma =
randn * 1e-3 as f16, with
* half of the rows scaled by 1e-3, so their f16 gradients are subnormal or underflow;
* every third ray's dL/dcolor zero (32-row tiles the pos pass keeps to itself);
* one of those rays with dL/dsigma zero too (tiles with no incoming gradient);
* one other ray with only dL/dsigma zero;
* rows whose f16 pre-activations lie within 2e-3 of a ReLU kink re-drawn, so that an f32
  and an f64 accumulation of the same layer cannot disagree on a mask.
"""

import functools

import torch

from oracle import ref_ingp, ref_tcnn

ARMS = ("f64", "f32", "f32rev")
SHAPES = [(64, 12), (40, 13), (1024, 3)]   # (n_per_ray, R): M = 768, 520, 3,072
LOSS_SCALE = 128.0


def _h(t):
    return t.half().double()


def min_preact(enc, dirs, n_per_ray, pp, pd, width, nhd, n_out):
    """min |pre-activation| per row over every ReLU of the field in f16 operands (hidden
    layers, sigma, the n_out colours): test_kernels_gpu._field_preacts for any n_out."""
    P0 = _h(pp[: 32 * width]).view(width, 32)
    P1 = _h(pp[32 * width:]).view(16, width)
    a0 = _h(enc) @ P0.T
    pos_out = _h(torch.relu(a0)) @ P1.T
    sh = torch.from_numpy(ref_tcnn.sh(dirs.repeat_interleave(n_per_ray, 0).numpy(), 2))
    x = torch.cat([_h(sh), _h(pos_out[:, 1:]), torch.ones(enc.shape[0], 13, dtype=torch.float64)], 1)
    off, mins = 0, [a0.abs().min(1).values, pos_out[:, 0].abs()]
    dims = [32] + [width] * nhd + [16]
    for k in range(nhd + 1):
        Wk = _h(pd[off: off + dims[k + 1] * dims[k]]).view(dims[k + 1], dims[k])
        off += dims[k + 1] * dims[k]
        a = x @ Wk.T
        mins.append(a.abs().min(1).values if k < nhd else a[:, :n_out].abs().min(1).values)
        x = _h(torch.relu(a))
    return torch.stack(mins, 1).min(1).values


def dir_layer_slices(width, nhd):
    """(name, slice) of each layer of the flat dir_mlp parameter vector (32 padded
    inputs, 16 padded outputs)."""
    sizes = [width * 32] + [width * width] * (nhd - 1) + [16 * width]
    out, off = [], 0
    for k, n in enumerate(sizes):
        out.append((f"dir_layer{k}", slice(off, off + n)))
        off += n
    return out


def make_inputs(width, nhd, n_out, n_per_ray, R):
    """CPU tensors: pp, pd (f32 flat parameters), enc (M, 32) f16, dirs (R, 3) f32,
    d_color (M, n_out) f16, d_sigma (M,) f16, and the special rays."""
    M = n_per_ray * R
    gen = torch.Generator().manual_seed(100000 * width + 10000 * nhd + 1000 * n_out + M)
    n_pp = 32 * width + 16 * width
    n_pd = sum(s.stop - s.start for _, s in dir_layer_slices(width, nhd))
    pp = torch.randn(n_pp, generator=gen) * (2.0 / 32) ** 0.5
    pd = torch.randn(n_pd, generator=gen) * (2.0 / width) ** 0.5
    enc = (torch.rand(M, 32, generator=gen) * 2 - 1).half()
    dirs = torch.rand(R, 3, generator=gen)
    for _ in range(60):
        tied = min_preact(enc.double(), dirs, n_per_ray, pp.double(), pd.double(), width, nhd,
                          n_out) < 2e-3
        if not tied.any():
            break
        enc[tied] = (torch.rand(int(tied.sum()), 32, generator=gen) * 2 - 1).half()
    assert not tied.any()
    dcol = torch.randn(M, n_out, generator=gen) * 1e-2
    dsig = torch.randn(M, generator=gen) * 1e-3
    tiny = torch.rand(M, generator=gen) < 0.5
    dcol[tiny] *= 1e-3
    dsig[tiny] *= 1e-3
    dcol, dsig = dcol.half(), dsig.half()
    ray = torch.arange(M) // n_per_ray
    dcol[ray % 3 == 0] = 0
    no_grad_ray = 0 if R <= 3 else 3      # dL/dcolor zero already; dL/dsigma too
    sigma_zero_ray = 1 if R <= 3 else 4   # dL/dcolor live, dL/dsigma zero
    dsig[ray == no_grad_ray] = 0
    dsig[ray == sigma_zero_ray] = 0
    return {"pp": pp, "pd": pd, "enc": enc, "dirs": dirs, "d_color": dcol, "d_sigma": dsig,
            "n_per_ray": n_per_ray, "R": R, "M": M, "width": width, "nhd": nhd, "n_out": n_out,
            "no_grad_ray": no_grad_ray, "sigma_zero_ray": sigma_zero_ray}


def tile_masks(inp):
    """Per 32-row tile, from the inputs: any nonzero dL/dcolor; any nonzero gradient."""
    M = inp["M"]
    pad = -M % 32
    c = torch.nn.functional.pad((inp["d_color"] != 0).any(1), (0, pad)).view(-1, 32).any(1)
    s = torch.nn.functional.pad(inp["d_sigma"] != 0, (0, pad)).view(-1, 32).any(1)
    return c, c | s


def run_oracle(inp, acc):
    """The helper's backward on the inputs: dL/denc (M, 32) f16, g_pos, g_dir (f64 values
    of tcnn's f16 parameter gradients)."""
    enc = inp["enc"].clone().requires_grad_(True)
    pp = inp["pp"].double().requires_grad_(True)
    pd = inp["pd"].double().requires_grad_(True)
    sigma, color = ref_ingp.field_reference(enc, inp["dirs"], inp["n_per_ray"], pp, pd,
                                            inp["width"], inp["nhd"], inp["n_out"], acc)
    assert sigma.dtype == torch.float16 and color.dtype == torch.float16
    assert sigma.shape == (inp["M"],) and color.shape == (inp["M"], inp["n_out"])
    torch.autograd.backward([color, sigma], [inp["d_color"], inp["d_sigma"]])
    assert enc.grad.dtype == torch.float16
    return {"d_enc": enc.grad, "g_pos": pp.grad, "g_dir": pd.grad}


@functools.lru_cache(maxsize=None)
def case(width, nhd, n_out, n_per_ray, R):
    """(inputs, {arm: oracle results}, arm spread) of one network and shape, evaluated once
    per process and shared by the tests; nobody writes to the tensors."""
    inp = make_inputs(width, nhd, n_out, n_per_ray, R)
    arms = {a: run_oracle(inp, a) for a in ARMS}
    return inp, arms, arm_spread(arms, width, nhd)


def rel(a, b):
    a, b = a.double(), b.double()
    return ((a - b).norm() / b.norm().clamp_min(1e-300)).item()


def arm_spread(arms, width, nhd):
    """The larger of the f32 / f32rev arms' relative L2 distances to the f64 arm, for
    dL/denc, g_pos, g_dir and each layer's slice of g_dir; the arms' disagreement on which
    rows are nonzero and the share of differing dL/denc elements."""
    ref = arms["f64"]
    out = {}
    for k in ("d_enc", "g_pos", "g_dir"):
        out[k] = max(rel(arms[a][k], ref[k]) for a in ("f32", "f32rev"))
    for name, sl in dir_layer_slices(width, nhd):
        out[name] = max(rel(arms[a]["g_dir"][sl], ref["g_dir"][sl]) for a in ("f32", "f32rev"))
    nz = (ref["d_enc"] != 0).any(1)
    out["row_disagree"] = max(((arms[a]["d_enc"] != 0).any(1) != nz).double().mean().item()
                              for a in ("f32", "f32rev"))
    out["elem_differ"] = max((arms[a]["d_enc"] != ref["d_enc"]).double().mean().item()
                             for a in ("f32", "f32rev"))
    return out
