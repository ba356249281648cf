"""Every reference-numerics entry form of the fused field backward (bwd_rt_kernel<..., F>,
the forms F with reference numerics, csrc/field_fused.hip) against the oracle's field chain in reference semantics
(oracle/ref_ingp.field_reference, f64 arm), on inputs where the dir network's backward does
nonzero work: live f16 dL/dcolor, about half of it subnormal once loss-scaled, mixed with
zero-colour tiles (pos pass), gradient-free tiles (skipped) and a ray with dL/dsigma alone
zero (tests/field_ref16_inputs.py; preconditions in test_field_ref16_oracle_cpu.py).

The bar of each comparison is 4x the oracle's own accumulation-order spread on the same
inputs (the larger relative L2 distance of its f32 / f32rev arms to the f64 arm; factor 4 as
in test_train_step_matches_oracle), never a figure taken from the kernel.

Measured on MI355X: relative L2 distance to the f64 arm at the shapes (64, 12) / (40, 13) /
(1024, 3), the largest of the six forms, which give the same dL/denc bit for bit and the same
parameter gradients up to the f32 atomic order; "ratio" is the largest distance / arm spread
over every quantity, dir layer, form and shape of the network (bar: 4).

    W, NHD, n_out   dL/denc                  g_pos                    g_dir                    ratio
    64, 2, 4        0      3.2e-5 1.6e-5     4.8e-6 4.1e-5 3.5e-5     1.2e-6 2.0e-5 1.2e-4     3.3
    64, 1, 4        4.3e-7 2.1e-5 2.1e-5     4.7e-7 1.2e-5 4.0e-5     4.6e-6 6.3e-7 2.5e-6     1.2
    32, 2, 4        0      3.1e-5 2.6e-7     7.6e-6 3.2e-5 0          1.7e-5 0      7.9e-6     1.0
    32, 1, 4        9.0e-6 8.2e-6 2.5e-5     0      4.4e-7 7.5e-5     0      5.1e-5 2.2e-5     1.1
    64, 2, 3        1.0e-5 1.3e-6 1.5e-5     6.0e-5 2.1e-6 2.6e-5     5.2e-5 7.4e-7 1.1e-5     0.8

The largest single dir-layer distance is 1.7e-4 (output layer, W = 64, NHD = 2, (1024, 3); its
spread 1.35e-4). The kernel's nonzero rows are the oracle's in every case (disagreement 0 of
768 / 520 / 3,072 rows), and with a workspace the list pass takes 16 of 24, 13 of 17 and 64
of 96 tiles. The distances are sums of single f16 roundings that fall the other way, so they
come in lumps: the ratio 3.3 is ONE element of g_pos (64, 12) whose f32 sum lies on an f16
rounding boundary (4.8e-6, against an arm spread of 1.5e-6 that is itself one smaller such
element); three of twelve launches had it on the oracle's side and measured 0.
"""

import ctypes

import pytest
import torch

from tests import field_ref16_inputs as fi

pytestmark = pytest.mark.gpu

FORMS = ("ref16", "tiles", "rows", "rows_ws", "rows_h", "rows_h_ws")
NETS = [(64, 2, 4), (64, 1, 4), (32, 2, 4), (32, 1, 4),
        (64, 2, 3)]   # 3 outputs: the general d_color layout (one kernel, no pos / list pass)


def _row_bits(d_enc):
    """Bit m % 32 of int32 word m // 32 set iff row m of d_enc has a nonzero value."""
    nz = (d_enc != 0).any(1).to(torch.int64).cpu()
    nz = torch.nn.functional.pad(nz, (0, -nz.numel() % 32)).view(-1, 32)
    w = (nz << torch.arange(32, dtype=torch.int64)[None]).sum(1)
    return torch.where(w >= 2**31, w - 2**32, w).to(torch.int32)


def _run_form(dev, form, inp, t):
    """One entry form on the device tensors t: dL/denc (M, 32) as stored, g_pos / g_dir after
    the pipeline's anr_grad_quantize_f16 (instant_ngp.py: _TcnnGradsAtBackwardEnd), row bits
    or tile flags, the list pass's tile count."""
    from atmonr_amd import _lib

    lib, s = _lib.load(), _lib.stream(dev)
    M, n_out, n_per_ray = inp["M"], inp["n_out"], inp["n_per_ray"]
    n_tiles = -(-M // 32)
    g_pos, g_dir = torch.zeros_like(t["pp"]), torch.zeros_like(t["pd"])
    half = form.startswith("rows_h")
    dc, ds = (t["dc16"], t["ds16"]) if half else (t["dc32"], t["ds32"])
    head = (t["pb"], t["db"], t["packed"].data_ptr(), t["enc"].data_ptr(), 32,
            t["dirs"].data_ptr(), n_per_ray, M, ds.data_ptr(), dc.data_ptr(), n_out)
    bits = flags = listed = None
    if form in ("ref16", "tiles"):
        d_enc = torch.full((M, 32), float("nan"), device=dev)
        tail = (d_enc.data_ptr(), 32, g_pos.data_ptr(), g_dir.data_ptr(), fi.LOSS_SCALE)
        if form == "tiles":
            flags = torch.full((n_tiles,), 7, device=dev, dtype=torch.uint8)
            _lib.call("anr_ingp_field_bwd_ref16_tiles", *head, *tail, flags.data_ptr(), s)
        else:
            _lib.call("anr_ingp_field_bwd_ref16", *head, *tail, s)
    else:
        d_enc = torch.full((M, 32), float("nan"), device=dev, dtype=torch.float16)
        bits = torch.full((n_tiles,), -7, device=dev, dtype=torch.int32)
        ws = form.endswith("_ws")
        wsb = lib.anr_ingp_field_bwd_ref16_rows_workspace_bytes(M) if ws else 0
        wst = torch.zeros(max(1, wsb), device=dev, dtype=torch.uint8)
        _lib.call("anr_ingp_field_bwd_ref16_rows_h" if half else "anr_ingp_field_bwd_ref16_rows",
                  *head, d_enc.data_ptr(), 32, g_pos.data_ptr(), g_dir.data_ptr(), fi.LOSS_SCALE,
                  bits.data_ptr(), wst.data_ptr() if ws else None, wsb, s)
        torch.cuda.synchronize(dev)
        if ws and n_out == 4:   # the fast layout: pos pass + list pass
            listed = int(wst[:4].view(torch.int32).item())
    for g in (g_pos, g_dir):
        _lib.call("anr_grad_quantize_f16", g.data_ptr(), g.numel(), fi.LOSS_SCALE, s)
    torch.cuda.synchronize(dev)
    return {"d_enc": d_enc.cpu(), "g_pos": g_pos.double().cpu(), "g_dir": g_dir.double().cpu(),
            "bits": None if bits is None else bits.cpu(),
            "flags": None if flags is None else flags.cpu(), "listed": listed}


@pytest.mark.parametrize("n_per_ray,R", fi.SHAPES)
@pytest.mark.parametrize("width,nhd,n_out", NETS)
def test_field_bwd_ref16_forms_match_oracle(dev, width, nhd, n_out, n_per_ray, R):
    from atmonr_amd import _lib

    inp, arms, spread = fi.case(width, nhd, n_out, n_per_ray, R)
    ref = arms["f64"]
    assert spread["row_disagree"] == 0.0
    M = inp["M"]
    n_tiles = -(-M // 32)
    colour_tiles, live_tiles = fi.tile_masks(inp)
    n_listed = int(colour_tiles.sum())
    assert 0 < n_listed < n_tiles          # the list pass has work, and so has the pos pass
    assert (~live_tiles).any()
    dead_rows = (~live_tiles).repeat_interleave(32)[:M]
    ref_nz = (ref["d_enc"] != 0).any(1)

    lib = _lib.load()
    pdsc = _lib.mlp_desc(32, 16, width, 1, False)
    ddsc = _lib.mlp_desc(19, n_out, width, nhd, False)
    pb, db = ctypes.byref(pdsc), ctypes.byref(ddsc)
    assert lib.anr_ingp_field_supported(pb, db) == 1
    assert lib.anr_mlp_n_params(pb) == inp["pp"].numel()
    assert lib.anr_mlp_n_params(db) == inp["pd"].numel()
    t = {"pb": pb, "db": db, "pp": inp["pp"].to(dev), "pd": inp["pd"].to(dev),
         "enc": inp["enc"].to(dev), "dirs": inp["dirs"].to(dev),
         "dc16": inp["d_color"].to(dev), "ds16": inp["d_sigma"].to(dev)}
    t["dc32"], t["ds32"] = t["dc16"].float(), t["ds16"].float()
    t["packed"] = torch.empty(lib.anr_ingp_field_packed_size(pb, db), device=dev,
                              dtype=torch.float16)
    _lib.call("anr_ingp_field_pack", pb, db, _lib.F16, t["pp"].data_ptr(), t["pd"].data_ptr(),
              t["packed"].data_ptr(), _lib.stream(dev))

    layers = fi.dir_layer_slices(width, nhd)
    print(f"W={width} NHD={nhd} n_out={n_out} n_per_ray={n_per_ray} R={R} arm spread:",
          {k: f"{v:.2e}" for k, v in spread.items()})
    failures = []
    for form in FORMS:
        out = _run_form(dev, form, inp, t)
        d = out["d_enc"]
        assert torch.isfinite(d.float()).all(), form
        rec = {"d_enc": fi.rel(d, ref["d_enc"]), "g_pos": fi.rel(out["g_pos"], ref["g_pos"]),
               "g_dir": fi.rel(out["g_dir"], ref["g_dir"])}
        for name, sl in layers:
            rec[name] = fi.rel(out["g_dir"][sl], ref["g_dir"][sl])
        rec["row_disagree"] = ((d != 0).any(1) != ref_nz).double().mean().item()
        print(f"  {form}:", {k: f"{v:.2e}" for k, v in rec.items()})
        # exact properties
        assert not d[dead_rows].any(), form
        assert torch.equal(d.half().float(), d.float()), form   # f16 numbers in either dtype
        if out["bits"] is not None:
            assert torch.equal(out["bits"], _row_bits(d)), form
        if out["flags"] is not None:
            assert torch.equal(out["flags"].bool(), live_tiles), form
        if out["listed"] is not None:
            assert out["listed"] == n_listed, (form, out["listed"], n_listed)
        # distances to the oracle, against its own spread
        for k in ["d_enc", "g_pos", "g_dir"] + [n for n, _ in layers]:
            if rec[k] > 4 * spread[k]:
                failures.append((form, k, rec[k], 4 * spread[k]))
        if rec["row_disagree"] > 1e-3:
            failures.append((form, "row_disagree", rec["row_disagree"], 1e-3))
    assert not failures, failures
