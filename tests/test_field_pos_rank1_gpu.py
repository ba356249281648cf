"""The pos pass of the reference-numerics field backward (bwd_rt_kernel<..., PosPass<Grads>>,
csrc/field_fused.hip) with its rank-1 output layer: dL/dpos_out of a zero-colour tile is
dL/dsigma in unit 0 and zeros elsewhere, so dL/dhidden is one f16 product per value
(P1[0][u] * dpo0) and only row 0 of dW_P1 is summed, both on the vector ALU instead of
MFMAs against 15 zero columns.

Each workspace form (``rows_ws``, ``rows_h_ws``: pos pass + list pass) runs against the
single-kernel form (``rows``, RefF16Rows, which keeps the MFMA arithmetic) and against
oracle/ref_ingp.field_reference (f64 arm):

* dL/denc, the row bits and the listed-tile count are exact (torch.equal / the count of
  tiles with a nonzero dL/dcolor in the inputs);
* g_pos, g_dir (and dL/denc) lie within 4x the oracle's own f32 / f32rev arm spread of the
  f64 arm, the bar of tests/test_field_ref16_oracle_gpu.py.

Shapes: M = 1, 33, 520 (40 x 13), 768 (64 x 12): the tail path, 16-row halves, a partial
last wave; M = 262,177 (11,399 x 23): waves own several tiles, so the deferred dL/denc
stores and the two-tile loop run. Inputs as in tests/field_ref16_inputs.py (f16 gradients,
half of the rows scaled into the subnormals, ReLU kinks re-drawn) with the tile classes
laid out per 32-row tile; the test asserts from the oracle's f64 forward, on the CPU, that
the inputs of each shape with more than one tile hold: zero-colour tiles next to listed
ones, a gradient-free tile, rows with sigma = 0 and a nonzero dL/dsigma, dL/dsigma whose
x128 product is an f16 subnormal, and open-density rows where P1[0][u] * dpo0 underflows to
zero for some units and not for others (three planted small weights in row 0 of P1).

Measured on MI355X, relative L2, shapes in the order above. dL/denc, row bits and the listed
count equal the single-kernel form's in every case, so its dL/denc distance to the f64 arm
is the single kernel's; "new to single" is the workspace forms' g_pos against the single
kernel's (after anr_grad_quantize_f16; 0 = every f16 parameter gradient the same).

    W, NHD       quantity            M = 1  33      520     768     262,177
    64, 2        arm spread d_enc    0      0       3.5e-5  1.6e-5  3.4e-5
                 arm spread g_pos    0      2.5e-6  3.8e-5  5.7e-5  9.6e-5
                 d_enc to f64        0      0       4.0e-5  2.2e-6  2.5e-5
                 g_pos to f64        0      0       5.5e-5  3.0e-6  6.5e-5
                 g_dir to f64        0      0       1.8e-5  2.0e-6  5.9e-5
                 g_pos new to single 0      0       0       3.0e-6  1.0e-5
    32, 1        arm spread d_enc    0      1.5e-5  9.6e-5  2.5e-5  1.9e-5
                 arm spread g_pos    0      0       7.7e-5  1.7e-5  6.6e-5
                 d_enc to f64        0      0       9.6e-5  1.3e-5  1.2e-5
                 g_pos to f64        0      0       7.4e-5  1.2e-5  3.5e-5
                 g_dir to f64        0      0       1.3e-4  1.6e-5  1.8e-5
                 g_pos new to single 0      0       1.6e-6  0       3.0e-6

The largest dL/denc or g_pos distance / spread ratio is 1.5 (bar 4). The parameter gradients come from f32
atomics, so the nonzero figures move from launch to launch by single f16 roundings.
"""

import ctypes
import functools

import pytest
import torch

from tests import field_ref16_inputs as fi
from tests.test_field_ref16_oracle_gpu import _row_bits, _run_form

pytestmark = pytest.mark.gpu

NETS = [(64, 2, 4), (32, 1, 4)]
SHAPES = [(1, 1), (33, 1), (40, 13), (64, 12), (11399, 23)]   # (n_per_ray, R)
FORMS = ("rows_ws", "rows_h_ws")


def _make_inputs(width, nhd, n_out, n_per_ray, R):
    """fi.make_inputs' distributions with the gradient classes laid out per 32-row tile:
    tile t has dL/dcolor zero unless t % 4 is 1 or 3, and no gradient at all when
    t % 8 == 2; three small weights planted in row 0 of P1."""
    M = n_per_ray * R
    gen = torch.Generator().manual_seed(7000000 + 100000 * width + 10000 * nhd + M)
    n_pp = 32 * width + 16 * width
    n_pd = sum(s.stop - s.start for _, s in fi.dir_layer_slices(width, nhd))
    pp = torch.randn(n_pp, generator=gen) * (2.0 / 32) ** 0.5
    pd = torch.randn(n_pd, generator=gen) * (2.0 / width) ** 0.5
    w1 = pp[32 * width:].view(16, width)
    w1[0, 3], w1[0, width // 2 + 1], w1[0, width - 5] = 2.0 ** -10, -(2.0 ** -9), 2.0 ** -12
    enc = (torch.rand(M, 32, generator=gen) * 2 - 1).half()
    dirs = torch.rand(R, 3, generator=gen)
    for _ in range(60):
        tied = fi.min_preact(enc.double(), dirs, n_per_ray, pp.double(), pd.double(), width,
                             nhd, n_out) < 2e-3
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
    tile = torch.arange(M) // 32
    dcol[(tile % 4 != 1) & (tile % 4 != 3)] = 0
    dsig[tile % 8 == 2] = 0
    return {"pp": pp, "pd": pd, "enc": enc, "dirs": dirs, "d_color": dcol, "d_sigma": dsig,
            "n_per_ray": n_per_ray, "R": R, "M": M, "width": width, "nhd": nhd, "n_out": n_out}


@functools.lru_cache(maxsize=None)
def _case(width, nhd, n_out, n_per_ray, R):
    inp = _make_inputs(width, nhd, n_out, n_per_ray, R)
    arms = {a: fi.run_oracle(inp, a) for a in fi.ARMS}
    return inp, arms, fi.arm_spread(arms, width, nhd)


def _assert_classes(inp):
    """The input classes the rank-1 path has to get right, from the f64 forward."""
    M, W = inp["M"], inp["width"]
    colour_tiles, live_tiles = fi.tile_masks(inp)
    assert colour_tiles.any() and (~colour_tiles & live_tiles).any()   # listed next to pos
    assert (~live_tiles).any()                                         # gradient-free tile
    pos_rows = (~colour_tiles).repeat_interleave(32)[:M]
    P0 = inp["pp"][: 32 * W].half().double().view(W, 32)
    P1 = inp["pp"][32 * W:].half().double().view(16, W)
    hp = torch.relu(inp["enc"].double() @ P0.T).half().double()
    sigma = torch.relu((hp @ P1.T)[:, 0]).half()
    ds = inp["d_sigma"]
    assert (pos_rows & (sigma == 0) & (ds != 0)).any()                 # dead density
    d0 = (ds.float() * fi.LOSS_SCALE).half()
    sub = (d0 != 0) & (d0.abs().float() < 2.0 ** -14)
    assert (pos_rows & sub).any()                                      # subnormal x128 product
    opened = pos_rows & (sigma > 0) & (d0 != 0)
    prod = (P1[0][None, :] * d0.double()[:, None])[opened]
    under = (prod != 0) & (prod.half() == 0)
    assert (under.any(1) & (prod.half() != 0).any(1)).any()            # partial underflow


@pytest.mark.parametrize("n_per_ray,R", SHAPES)
@pytest.mark.parametrize("width,nhd,n_out", NETS)
def test_pos_pass_rank1_matches_single_kernel_and_oracle(dev, width, nhd, n_out, n_per_ray, R):
    from atmonr_amd import _lib

    inp, arms, spread = _case(width, nhd, n_out, n_per_ray, R)
    ref = arms["f64"]
    M = inp["M"]
    colour_tiles, live_tiles = fi.tile_masks(inp)
    n_listed = int(colour_tiles.sum())
    if M >= 256:
        _assert_classes(inp)
    else:   # M = 1: the pos pass's tile; M = 33: that and a listed one-row tile
        assert n_listed == (M > 32) and live_tiles.all() and not colour_tiles[0]

    lib = _lib.load()
    pdsc = _lib.mlp_desc(32, 16, width, 1, False)
    ddsc = _lib.mlp_desc(19, n_out, width, nhd, False)
    pb, db = ctypes.byref(pdsc), ctypes.byref(ddsc)
    assert lib.anr_ingp_field_supported(pb, db) == 1
    t = {"pb": pb, "db": db, "pp": inp["pp"].to(dev), "pd": inp["pd"].to(dev),
         "enc": inp["enc"].to(dev), "dirs": inp["dirs"].to(dev),
         "dc16": inp["d_color"].to(dev), "ds16": inp["d_sigma"].to(dev)}
    t["dc32"], t["ds32"] = t["dc16"].float(), t["ds16"].float()
    t["packed"] = torch.empty(lib.anr_ingp_field_packed_size(pb, db), device=dev,
                              dtype=torch.float16)
    _lib.call("anr_ingp_field_pack", pb, db, _lib.F16, t["pp"].data_ptr(), t["pd"].data_ptr(),
              t["packed"].data_ptr(), _lib.stream(dev))

    single = _run_form(dev, "rows", inp, t)
    assert torch.equal(single["bits"], _row_bits(single["d_enc"]))
    print(f"W={width} NHD={nhd} M={M} listed {n_listed} of {-(-M // 32)} tiles; arm spread:",
          {k: f"{spread[k]:.2e}" for k in ("d_enc", "g_pos", "g_dir")})
    print("  rows (single kernel) to f64:",
          {k: f"{fi.rel(single[k], ref[k]):.2e}" for k in ("d_enc", "g_pos", "g_dir")})
    failures = []
    for form in FORMS:
        out = _run_form(dev, form, inp, t)
        rec = {k: fi.rel(out[k], ref[k]) for k in ("d_enc", "g_pos", "g_dir")}
        rec["g_pos_to_single"] = fi.rel(out["g_pos"], single["g_pos"])
        print(f"  {form} to f64:", {k: f"{v:.2e}" for k, v in rec.items()})
        assert torch.equal(out["d_enc"], single["d_enc"]), form
        assert torch.equal(out["bits"], single["bits"]), form
        assert out["listed"] == n_listed, (form, out["listed"], n_listed)
        for k in ("d_enc", "g_pos", "g_dir"):
            if rec[k] > 4 * spread[k]:
                failures.append((form, k, rec[k], 4 * spread[k]))
    assert not failures, failures
