"""The fused Instant-NGP field with S = 2..4 density outputs (multi_band_extinction),
through the C ABI: anr_ingp_field_{pack,fwd,density,bwd} on a dir network of 20 - S inputs.

The oracle is local and in f64 (the style of _field_ref / _field_preacts in
tests/test_kernels_gpu.py, with S as a parameter): sigma = relu(pos_out[:, :S]), the dir
input [SH2 | pos_out[:, S:] | 1.0 padding], a first dir layer of (W, n_input_padded)
parameters (32 wide for S <= 3, 16 wide for S = 4), operands rounded where the kernel
rounds them. Tolerances are test_ingp_field_matches_oracle's: f16 1e-2 forward / 2e-2
gradients, bf16 2e-2 / 5e-2, relative to the largest value."""

import ctypes
import functools

import pytest
import torch

from oracle import ref_tcnn
from tests.test_kernels_gpu import close

pytestmark = pytest.mark.gpu

NB, N_PER_RAY = 4, 37


def _descs(S, width, nhd):
    from atmonr_amd import _lib

    return _lib.mlp_desc(32, 16, width, 1, False), _lib.mlp_desc(20 - S, NB, width, nhd, False)


def _field_ref(enc, dirs, n_per_ray, pp, pd, width, nhd, S, half):
    """sigma (M, S), colour of instant_ngp.py:163-184 with multi_band_extinction, f64 with
    the kernel's roundings (half=True: f16; "bf16": bf16 operands)."""
    pos_out = ref_tcnn.mlp_fwd(enc, pp, 32, 16, width, 1, half=half)
    sh = torch.from_numpy(ref_tcnn.sh(dirs.detach().repeat_interleave(n_per_ray, 0).numpy(), 2))
    x = torch.cat([sh, pos_out[:, S:]], dim=1)
    color = ref_tcnn.mlp_fwd(x, pd, 20 - S, NB, width, nhd, output_relu=True, half=half)
    return torch.relu(pos_out[:, :S]), color


def _field_preacts(enc, dirs, n_per_ray, pp, pd, width, nhd, S, half):
    """min |pre-activation| per row over every ReLU of the field, the S density units
    included (tie detector)."""
    h = ref_tcnn.rounder(half)
    nip = (20 - S + 15) // 16 * 16
    P0 = h(pp[: 32 * width]).view(width, 32)
    P1 = h(pp[32 * width:]).view(16, width)
    a0 = h(enc) @ P0.T
    pos_out = h(torch.relu(a0)) @ P1.T
    sh = torch.from_numpy(ref_tcnn.sh(dirs.repeat_interleave(n_per_ray, 0).numpy(), 2))
    x = torch.cat([h(sh), h(pos_out[:, S:]),
                   torch.ones(enc.shape[0], nip - (20 - S), dtype=torch.float64)], 1)
    off, hcur = 0, x
    mins = [a0.abs().min(1).values, pos_out[:, :S].abs().min(1).values]
    dims = [nip] + [width] * nhd + [16]
    for k in range(nhd + 1):
        Wk = h(pd[off: off + dims[k + 1] * dims[k]]).view(dims[k + 1], dims[k])
        off += dims[k + 1] * dims[k]
        a = hcur @ Wk.T
        mins.append(a.abs().min(1).values if k < nhd else a[:, :NB].abs().min(1).values)
        hcur = h(torch.relu(a))
    return torch.stack(mins, 1).min(1).values


@functools.lru_cache(maxsize=None)
def _case(S, width, nhd, R, mma):
    """Inputs (CPU) and the f64 oracle's outputs of one case, computed once and left
    unchanged: the autograd graph stays, so the tests ask it for the gradients they need."""
    from atmonr_amd import _lib

    half = "bf16" if mma == "bf16" else True
    M = N_PER_RAY * R
    gen = torch.Generator().manual_seed(100000 * S + 1000 * width + 10 * nhd + R)
    pdsc, ddsc = _descs(S, width, nhd)
    lib = _lib.load()
    n_pp = lib.anr_mlp_n_params(ctypes.byref(pdsc))
    n_pd = lib.anr_mlp_n_params(ctypes.byref(ddsc))
    pp = torch.randn(n_pp, generator=gen) * (2.0 / 32) ** 0.5
    pd = torch.randn(n_pd, generator=gen) * (2.0 / width) ** 0.5
    enc = torch.rand(M, 32, generator=gen) * 2 - 1
    dirs = torch.nn.functional.normalize(torch.randn(R, 3, generator=gen), dim=1)
    for _ in range(40):  # keep every ReLU input away from 0 (16-bit kernel vs f64 oracle)
        tied = _field_preacts(enc, dirs, N_PER_RAY, pp, pd, width, nhd, S, half) < 2e-3
        if not tied.any():
            break
        enc[tied] = torch.rand(int(tied.sum()), 32, generator=gen) * 2 - 1
    assert not tied.any()
    enc_h = enc.half()
    e64 = enc_h.double().requires_grad_(True)
    pr_p = pp.double().requires_grad_(True)
    pr_d = pd.double().requires_grad_(True)
    rs, rc = _field_ref(e64, dirs, N_PER_RAY, pr_p, pr_d, width, nhd, S, half)
    dcol = torch.randn(M, NB, generator=gen) * 1e-2
    # one seed per band, so a swapped band shows
    dsig = torch.stack([torch.randn(M, generator=torch.Generator().manual_seed(7000 + 13 * j + R))
                        for j in range(S)], 1) * 1e-3
    return dict(pp=pp, pd=pd, enc_h=enc_h, dirs=dirs, dcol=dcol, dsig=dsig, e64=e64, pr_p=pr_p,
                pr_d=pr_d, rs=rs, rc=rc, n_pp=n_pp, n_pd=n_pd, M=M)


def _pack(lib, dev, pb, db, code, pp_d, pd_d):
    from atmonr_amd import _lib

    packed = torch.empty(lib.anr_ingp_field_packed_size(pb, db), device=dev, dtype=torch.float16)
    _lib.call("anr_ingp_field_pack", pb, db, code, pp_d.data_ptr(), pd_d.data_ptr(),
              packed.data_ptr(), _lib.stream(dev))
    return packed


def _bwd(lib, dev, pb, db, code, packed, enc, ld, dirs, n_per_ray, M, dsig, dcol, d_enc, g_pos,
         g_dir):
    from atmonr_amd import _lib

    ws_bytes = lib.anr_ingp_field_bwd_workspace_bytes(pb, db, code, M)
    assert (ws_bytes == 0) == (code == _lib.BF16)
    ws = torch.empty(max(1, ws_bytes // 4), device=dev)
    _lib.call("anr_ingp_field_bwd", pb, db, code, packed.data_ptr(), enc.data_ptr(), ld,
              dirs.data_ptr(), n_per_ray, M, dsig.data_ptr(), dcol.data_ptr(), NB,
              d_enc.data_ptr(), 32, g_pos.data_ptr(), g_dir.data_ptr(),
              ws.data_ptr() if ws_bytes else None, ws_bytes, _lib.stream(dev))


@pytest.mark.parametrize("mma", ["f16", "bf16"])
@pytest.mark.parametrize("R", [29, 300])
@pytest.mark.parametrize("width,nhd", [(64, 2), (32, 1)])
@pytest.mark.parametrize("S", [4, 2, 3])
def test_multiband_field_matches_oracle(dev, S, width, nhd, R, mma):
    """Forward and backward against the oracle: sigma (M, S), colour, dL/denc and both
    parameter gradients (accumulated into non-zero buffers). 37 samples per ray on 29 / 300
    rays: ragged 16- and 32-row tiles, more than one tile per wavefront. S = 4 and 2 are the
    two parameter layouts (16- and 32-wide first dir layer); S = 3 is the 12-byte store.
    Pad columns: for S <= 3 the gradient of every padding column of the first dir layer
    equals the oracle's; for S = 4 g_dir has exactly anr_mlp_n_params entries and nothing
    is written behind them.
    On the code before multi-band: anr_ingp_field_supported returned 0 and the forward -1."""
    from atmonr_amd import _lib

    code = _lib.BF16 if mma == "bf16" else _lib.F16
    rf, rb = (2e-2, 5e-2) if mma == "bf16" else (1e-2, 2e-2)
    c = _case(S, width, nhd, R, mma)
    M, n_pp, n_pd = c["M"], c["n_pp"], c["n_pd"]
    lib = _lib.load()
    pdsc, ddsc = _descs(S, width, nhd)
    pb, db = ctypes.byref(pdsc), ctypes.byref(ddsc)
    assert lib.anr_ingp_field_supported(pb, db) == 1
    nip = 16 if S == 4 else 32
    assert ddsc.n_input_padded == nip
    assert n_pd == nip * width + (nhd - 1) * width * width + 16 * width
    s = _lib.stream(dev)
    pp_d, pd_d = c["pp"].to(dev), c["pd"].to(dev)
    enc_d, dirs_d = c["enc_h"].to(dev), c["dirs"].to(dev)
    packed = _pack(lib, dev, pb, db, code, pp_d, pd_d)
    sigma = torch.full((M + 1, S), float("nan"), device=dev)
    color = torch.empty(M, NB, device=dev)
    _lib.call("anr_ingp_field_fwd", pb, db, code, packed.data_ptr(), enc_d.data_ptr(), 32,
              dirs_d.data_ptr(), N_PER_RAY, M, sigma.data_ptr(), color.data_ptr(), NB, s)
    assert torch.isnan(sigma[M]).all()  # nothing past row M
    rs, rc = c["rs"], c["rc"]
    assert (rs.detach() > 0).any(0).all()  # every band has live densities
    print(f"sigma err {(sigma[:M].double().cpu() - rs.detach()).abs().max().item():.3e} of "
          f"{rs.detach().abs().max().item():.3e}; colour err "
          f"{(color.double().cpu() - rc.detach()).abs().max().item():.3e} of "
          f"{rc.detach().abs().max().item():.3e}")
    close(sigma[:M], rs.detach(), rel=rf, atol=1e-4)
    close(color, rc.detach(), rel=rf, atol=1e-4)

    dcol, dsig = c["dcol"], c["dsig"]
    g_enc, g_p, g_d = torch.autograd.grad(
        (rc * dcol.double()).sum() + (rs * dsig.double()).sum(),
        (c["e64"], c["pr_p"], c["pr_d"]), retain_graph=True)
    dcol_d, dsig_d = dcol.to(dev), dsig.to(dev)
    d_enc = torch.full((M, 32), float("nan"), device=dev)
    guard = 64
    g_pos = torch.full((n_pp,), 0.5, device=dev)  # accumulated into
    g_dir = torch.full((n_pd + guard,), -0.25, device=dev)
    _bwd(lib, dev, pb, db, code, packed, enc_d, 32, dirs_d, N_PER_RAY, M, dsig_d, dcol_d, d_enc,
         g_pos, g_dir)
    for name, a, b in (("d_enc", d_enc, g_enc), ("g_pos", g_pos - 0.5, g_p),
                       ("g_dir", g_dir[:n_pd] + 0.25, g_d)):
        print(f"{name}: err {(a.double().cpu() - b).abs().max().item():.3e} of "
              f"{b.abs().max().item():.3e}")
    close(d_enc, g_enc, rel=rb, atol=1e-7)
    close(g_pos - 0.5, g_p, rel=rb, atol=1e-7)
    close(g_dir[:n_pd] + 0.25, g_d, rel=rb, atol=1e-7)
    assert torch.equal(g_dir[n_pd:], torch.full((guard,), -0.25, device=dev))
    if S < 4:  # the 12 + S trainable padding columns (input 1.0) of the first dir layer
        pad = (g_dir[: 32 * width] + 0.25).view(width, 32)[:, 20 - S:]
        pad_ref = g_d[: 32 * width].view(width, 32)[:, 20 - S:]
        assert pad_ref.abs().max() > 0
        # every padding column sees the same input, so the oracle's columns are equal and
        # each of the kernel's must match (a slot mapped twice or not at all would not)
        assert (pad_ref - pad_ref[:, :1]).abs().max() <= 1e-12 * pad_ref.abs().max()
        close(pad, pad_ref, rel=rb, atol=1e-7)


@pytest.mark.parametrize("mma", ["f16", "bf16"])
@pytest.mark.parametrize("S", [4, 2, 3])
def test_multiband_bwd_without_density_gradient(dev, S, mma):
    """No d_sigma: the backward's general d_color layout at S > 1 (the other cases here pass
    one and run the fast layout). dL/denc and both parameter gradients against the oracle's
    for the colour term alone, same tolerances as test_multiband_field_matches_oracle."""
    from atmonr_amd import _lib

    width, nhd, R = 64, 2, 29
    code = _lib.BF16 if mma == "bf16" else _lib.F16
    rb = 5e-2 if mma == "bf16" else 2e-2
    c = _case(S, width, nhd, R, mma)
    M, n_pp, n_pd = c["M"], c["n_pp"], c["n_pd"]
    lib = _lib.load()
    pdsc, ddsc = _descs(S, width, nhd)
    pb, db = ctypes.byref(pdsc), ctypes.byref(ddsc)
    pp_d, pd_d = c["pp"].to(dev), c["pd"].to(dev)
    enc_d, dirs_d = c["enc_h"].to(dev), c["dirs"].to(dev)
    packed = _pack(lib, dev, pb, db, code, pp_d, pd_d)
    g_enc, g_p, g_d = torch.autograd.grad((c["rc"] * c["dcol"].double()).sum(),
                                          (c["e64"], c["pr_p"], c["pr_d"]), retain_graph=True)
    dcol_d = c["dcol"].to(dev)
    d_enc = torch.full((M, 32), float("nan"), device=dev)
    g_pos, g_dir = torch.zeros(n_pp, device=dev), torch.zeros(n_pd, device=dev)
    ws_bytes = lib.anr_ingp_field_bwd_workspace_bytes(pb, db, code, M)
    ws = torch.empty(max(1, ws_bytes // 4), device=dev)
    _lib.call("anr_ingp_field_bwd", pb, db, code, packed.data_ptr(), enc_d.data_ptr(), 32,
              dirs_d.data_ptr(), N_PER_RAY, M, None, dcol_d.data_ptr(), NB, d_enc.data_ptr(), 32,
              g_pos.data_ptr(), g_dir.data_ptr(), ws.data_ptr() if ws_bytes else None, ws_bytes,
              _lib.stream(dev))
    close(d_enc, g_enc, rel=rb, atol=1e-7)
    close(g_pos, g_p, rel=rb, atol=1e-7)
    close(g_dir, g_d, rel=rb, atol=1e-7)


def test_multiband_one_band_at_a_time(dev):
    """d_color = 0 and d_sigma nonzero in band j only: dL/denc is the oracle's for that band
    alone, and differs between bands (S = 4, W = 64, two dir hidden layers, f16)."""
    from atmonr_amd import _lib

    S, width, nhd, R = 4, 64, 2, 29
    c = _case(S, width, nhd, R, "f16")
    M, n_pp, n_pd = c["M"], c["n_pp"], c["n_pd"]
    lib = _lib.load()
    pdsc, ddsc = _descs(S, width, nhd)
    pb, db = ctypes.byref(pdsc), ctypes.byref(ddsc)
    pp_d, pd_d = c["pp"].to(dev), c["pd"].to(dev)
    enc_d, dirs_d = c["enc_h"].to(dev), c["dirs"].to(dev)
    packed = _pack(lib, dev, pb, db, _lib.F16, pp_d, pd_d)
    dcol_d = torch.zeros(M, NB, device=dev)
    got, want = [], []
    for j in range(S):
        dsig = torch.zeros(M, S)
        dsig[:, j] = c["dsig"][:, j]
        (g_enc,) = torch.autograd.grad((c["rs"] * dsig.double()).sum(), (c["e64"],),
                                       retain_graph=True)
        dsig_d = dsig.to(dev)
        d_enc = torch.full((M, 32), float("nan"), device=dev)
        g_pos, g_dir = torch.zeros(n_pp, device=dev), torch.zeros(n_pd, device=dev)
        _bwd(lib, dev, pb, db, _lib.F16, packed, enc_d, 32, dirs_d, N_PER_RAY, M, dsig_d, dcol_d,
             d_enc, g_pos, g_dir)
        assert g_enc.abs().max() > 0
        close(d_enc, g_enc, rel=2e-2, atol=1e-9)
        assert g_dir.abs().max().item() == 0.0  # no colour gradient: nothing for the dir net
        got.append(d_enc.double().cpu())
        want.append(g_enc)
    for i in range(S):
        for j in range(i + 1, S):
            assert (got[i] - got[j]).abs().max() > 0.1 * max(want[i].abs().max(),
                                                             want[j].abs().max())


@pytest.mark.parametrize("mma", ["f16", "bf16"])
@pytest.mark.parametrize("M", [1, 77, 1000])
@pytest.mark.parametrize("S,width,nhd", [(4, 64, 2), (2, 32, 1), (3, 64, 1)])
def test_multiband_density_equals_field_sigma(dev, S, width, nhd, M, mma):
    """anr_ingp_field_density returns exactly the forward's sigma (M, S)."""
    from atmonr_amd import _lib

    code = _lib.BF16 if mma == "bf16" else _lib.F16
    g = torch.Generator(device=dev).manual_seed(width + M + S)
    lib = _lib.load()
    pdsc, ddsc = _descs(S, width, nhd)
    pb, db = ctypes.byref(pdsc), ctypes.byref(ddsc)
    pp = torch.randn(lib.anr_mlp_n_params(pb), device=dev, generator=g) * (2.0 / 32) ** 0.5
    pd = torch.randn(lib.anr_mlp_n_params(db), device=dev, generator=g) * (2.0 / width) ** 0.5
    enc = (torch.rand(M, 32, device=dev, generator=g) * 2 - 1).half()
    s = _lib.stream(dev)
    packed = _pack(lib, dev, pb, db, code, pp, pd)
    dirs = torch.full((1, 3), 0.5, device=dev)
    sig_full = torch.full((M, S), -1.0, device=dev)
    color = torch.empty(M, NB, device=dev)
    _lib.call("anr_ingp_field_fwd", pb, db, code, packed.data_ptr(), enc.data_ptr(), 32,
              dirs.data_ptr(), M, M, sig_full.data_ptr(), color.data_ptr(), NB, s)
    sig = torch.full((M + 1, S), -1.0, device=dev)
    _lib.call("anr_ingp_field_density", pb, db, code, packed.data_ptr(), enc.data_ptr(), 32, M,
              sig.data_ptr(), s)
    assert torch.equal(sig[:M], sig_full)
    assert (sig[M] == -1.0).all() and (sig_full >= 0).all()
    if M > 1:
        assert (sig_full > 0).any(0).all()


@pytest.mark.parametrize("mma", ["f16", "bf16"])
@pytest.mark.parametrize("S", [4, 2, 3])
def test_multiband_enc_quad_planes_equal_rows(dev, S, mma):
    """Row layout against level-quad planes (enc_stride = -plane) at M = 37 * 29: bit-identical
    sigma, colour, density and dL/denc; parameter gradients up to the atomic flush order.
    The uniform-tile forward (48 samples per ray) and the general one (37) both run, and at
    48 per ray the uniform-tile form's sigma and colour are bit-identical to the general
    form's (anr_ingp_field_force_fwd(0); test_multiband_field_matches_oracle holds that one
    to the oracle), as test_field_fwd_uniform_tile_matches_general asks at S = 1."""
    from atmonr_amd import _lib

    width, nhd = 64, 2
    code = _lib.BF16 if mma == "bf16" else _lib.F16
    lib = _lib.load()
    pdsc, ddsc = _descs(S, width, nhd)
    pb, db = ctypes.byref(pdsc), ctypes.byref(ddsc)
    s = _lib.stream(dev)
    for n_per_ray, R in ((37, 29), (48, 23)):
        M = n_per_ray * R
        g = torch.Generator(device=dev).manual_seed(21 + S)
        pp = torch.randn(lib.anr_mlp_n_params(pb), device=dev, generator=g) * (2.0 / 32) ** 0.5
        pd = torch.randn(lib.anr_mlp_n_params(db), device=dev, generator=g) * (2.0 / width) ** 0.5
        enc = (torch.rand(M, 32, device=dev, generator=g) * 2 - 1).half()
        plane = 8 * M + 24
        planes = torch.zeros(4 * plane, device=dev, dtype=torch.float16)
        for q in range(4):
            planes[q * plane:q * plane + 8 * M] = enc[:, 8 * q:8 * q + 8].reshape(-1)
        dirs = torch.rand(R + 1, 3, device=dev, generator=g)
        packed = _pack(lib, dev, pb, db, code, pp, pd)
        dcol = torch.randn(M, NB, device=dev, generator=g) * 1e-2
        dsig = torch.randn(M, S, device=dev, generator=g) * 1e-3
        out = {}
        for name, base, ld in (("rows", enc, 32), ("planes", planes, -plane)):
            sigma = torch.full((M + 4, S), float("nan"), device=dev)
            color = torch.empty(M, NB, device=dev)
            _lib.call("anr_ingp_field_fwd", pb, db, code, packed.data_ptr(), base.data_ptr(), ld,
                      dirs.data_ptr(), n_per_ray, M, sigma.data_ptr(), color.data_ptr(), NB, s)
            dens = torch.empty(M, S, device=dev)
            _lib.call("anr_ingp_field_density", pb, db, code, packed.data_ptr(), base.data_ptr(),
                      ld, M, dens.data_ptr(), s)
            d_enc = torch.empty(M, 32, device=dev)
            g_pos, g_dir = torch.zeros_like(pp), torch.zeros_like(pd)
            _bwd(lib, dev, pb, db, code, packed, base, ld, dirs, n_per_ray, M, dsig, dcol, d_enc,
                 g_pos, g_dir)
            assert torch.isnan(sigma[M:]).all() and torch.isfinite(sigma[:M]).all()
            out[name] = (sigma[:M], color, dens, d_enc, g_pos, g_dir)
        assert torch.equal(out["rows"][0], out["rows"][2])
        prev = lib.anr_ingp_field_force_fwd(0)
        try:
            sigma = torch.full((M + 4, S), float("nan"), device=dev)
            color = torch.empty(M, NB, device=dev)
            _lib.call("anr_ingp_field_fwd", pb, db, code, packed.data_ptr(), enc.data_ptr(), 32,
                      dirs.data_ptr(), n_per_ray, M, sigma.data_ptr(), color.data_ptr(), NB, s)
            torch.cuda.synchronize(dev)
        finally:
            lib.anr_ingp_field_force_fwd(prev)
        assert torch.isnan(sigma[M:]).all()
        assert torch.equal(sigma[:M], out["rows"][0]) and torch.equal(color, out["rows"][1])
        for a, b in zip(out["rows"][:4], out["planes"][:4]):
            assert torch.equal(a, b)
        for a, b in zip(out["rows"][4:], out["planes"][4:]):
            assert (a - b).abs().max().item() <= 2e-5 * b.abs().max().item()


@pytest.mark.parametrize("mma", ["f16", "bf16"])
@pytest.mark.parametrize("width,nhd", [(64, 2), (32, 1)])
def test_multiband_bwd_relaunch_deterministic(dev, width, nhd, mma):
    """The hazard guard of test_ingp_field_bwd_relaunch_deterministic at S = 4: 12 launches
    of the backward on the same inputs give bit-identical dL/denc and parameter gradients
    within 2e-5 of the largest (the atomic flush order)."""
    from atmonr_amd import _lib

    S, R, n_per_ray = 4, 64, 64
    M = R * n_per_ray + 29
    code = _lib.BF16 if mma == "bf16" else _lib.F16
    g = torch.Generator(device=dev).manual_seed(width + nhd)
    lib = _lib.load()
    pdsc, ddsc = _descs(S, width, nhd)
    pb, db = ctypes.byref(pdsc), ctypes.byref(ddsc)
    pp = torch.randn(lib.anr_mlp_n_params(pb), device=dev, generator=g) * (2.0 / 32) ** 0.5
    pd = torch.randn(lib.anr_mlp_n_params(db), device=dev, generator=g) * (2.0 / width) ** 0.5
    enc = (torch.rand(M, 32, device=dev, generator=g) * 2 - 1).half()
    dirs = torch.rand(R + 1, 3, device=dev, generator=g)
    packed = _pack(lib, dev, pb, db, code, pp, pd)
    dcol = torch.randn(M, NB, device=dev, generator=g) * 1e-2
    dsig = torch.randn(M, S, device=dev, generator=g) * 1e-3
    first = None
    for _ in range(12):
        d_enc = torch.empty(M, 32, device=dev)
        g_pos, g_dir = torch.zeros_like(pp), torch.zeros_like(pd)
        _bwd(lib, dev, pb, db, code, packed, enc, 32, dirs, n_per_ray, M, dsig, dcol, d_enc,
             g_pos, g_dir)
        if first is None:
            first = (d_enc, g_pos, g_dir)
            continue
        assert torch.equal(d_enc, first[0])
        for a, b in ((g_pos, first[1]), (g_dir, first[2])):
            assert (a - b).abs().max().item() <= 2e-5 * b.abs().max().item()


def test_multiband_refusals_and_empty(dev):
    """The entries that stay at one density output answer an S = 4 pair with
    ANR_E_UNSUPPORTED before they look at a pointer; M = 0 returns 0 everywhere."""
    from atmonr_amd import _lib

    lib = _lib.load()
    UNSUPPORTED = -3
    pdsc, ddsc = _descs(4, 64, 2)
    pb, db = ctypes.byref(pdsc), ctypes.byref(ddsc)
    gdsc = _lib.hashgrid_desc(3, 16, 2, 16, 1.3819, 19)

    def calls(M):
        return {
            "fwd_h": lambda: lib.anr_ingp_field_fwd_h(pb, db, _lib.F16, None, None, 32, None, 1, M, None,
                                              None, 4, None),
            "fwd_rows": lambda: lib.anr_ingp_field_fwd_rows(pb, db, _lib.F16, None, None, 32, None, 1, M,
                                                    None, None, None, 4, None),
            "bwd_rows": lambda: lib.anr_ingp_field_bwd_rows(pb, db, _lib.F16, None, None, 32, None, 1, M,
                                                    None, None, None, 4, None, 32, None, None,
                                                    None, 0, None),
            "ref16": lambda: lib.anr_ingp_field_bwd_ref16(pb, db, None, None, 32, None, 1, M, None, None,
                                                  4, None, 32, None, None, 128.0, None),
            "ref16_tiles": lambda: lib.anr_ingp_field_bwd_ref16_tiles(pb, db, None, None, 32, None, 1, M,
                                                              None, None, 4, None, 32, None, None,
                                                              128.0, None, None),
            "ref16_rows": lambda: lib.anr_ingp_field_bwd_ref16_rows(pb, db, None, None, 32, None, 1, M,
                                                            None, None, 4, None, 32, None, None,
                                                            128.0, None, None, 0, None),
            "ref16_rows_h": lambda: lib.anr_ingp_field_bwd_ref16_rows_h(pb, db, None, None, 32, None, 1,
                                                                M, None, None, 4, None, 32, None,
                                                                None, 128.0, None, None, 0, None),
            "hash_field": lambda: lib.anr_ingp_hash_field_fwd(ctypes.byref(gdsc), None, M, None, _lib.F16,
                                                      None, 8 * max(M, 1), pb, db, _lib.F16, None,
                                                      None, 64, None, None, 4, None),
        }

    for name, fn in calls(10).items():
        rc = fn()
        assert rc == UNSUPPORTED, (name, rc)
        assert b"density output" in lib.anr_last_error(), name
    for name, fn in calls(0).items():
        if name in ("ref16_tiles", "ref16_rows", "ref16_rows_h"):
            continue  # these check their own extra pointers before M (as for S = 1)
        assert fn() == 0, name
    # the entries that take S > 1: empty launches
    assert lib.anr_ingp_field_fwd(pb, db, _lib.F16, None, None, 32, None, 1, 0, None, None, 4,
                                  None) == 0
    assert lib.anr_ingp_field_density(pb, db, _lib.F16, None, None, 32, 0, None, None) == 0
    assert lib.anr_ingp_field_bwd(pb, db, _lib.F16, None, None, 32, None, 1, 0, None, None, 4,
                                  None, 32, None, None, None, 0, None) == 0
