"""Argument handling of the fused-field entry points, without a GPU.

Every call here is answered by validation: a failed check, or the ``M == 0`` / ``B == 0``
early return. None reaches a kernel launch or an occupancy query, so the pointers are fake
addresses that are never dereferenced. Each case pins the status code and a distinguishing
part of ``anr_last_error()``; the order of the checks shows in which one answers.

Two checks of the shared backward cannot be reached through the C ABI and have no case:
"reference numerics need f16 MMA and dense rows" (every ``ref16*`` entry passes f16 and no
row list) and "f16 gradients need the f16-rows form" (``_ref16_rows_h`` refuses a null
``d_enc`` itself, first).
"""

import ctypes

import pytest

FAKE = 0x10000  # non-null, 256-byte aligned, never dereferenced
OK, INVALID, UNSUPPORTED = 0, -1, -3
M0 = 64  # rows of a case that does not set M


def _lib():
    from atmonr_amd import _lib

    return _lib


def _pair(S=1, n_out=4, width=64, nhd=2, dir_width=None):
    """pos / dir descriptors of a pair with S density outputs (dir inputs 20 - S)."""
    L = _lib()
    pos = L.mlp_desc(32, 16, width, 1, False)
    dird = L.mlp_desc(20 - S, n_out, dir_width or width, nhd, False)
    return pos, dird


def _grid(**fields):
    g = _lib().hashgrid_desc(3, 16, 2, 16, 1.3819, 19)
    for k, v in fields.items():
        setattr(g, k, v)
    return g


def _defaults():
    L = _lib()
    pos, dird = _pair()
    return dict(
        pos=pos, dir=dird, mma=L.F16, packed=FAKE, enc=FAKE, enc_stride=32, dirs=FAKE, npr=1,
        M=M0, rows=FAKE, sigma=FAKE, color=FAKE, color_stride=4, d_sigma=FAKE, d_color=FAKE,
        d_color_stride=4, d_enc=FAKE, d_enc_stride=32, g_pos=FAKE, g_dir=FAKE, ws=FAKE,
        ws_bytes=1 << 30, loss_scale=128.0, tile_nz=FAKE, row_nz=FAKE,
        # pack
        pos_params=FAKE, dir_params=FAKE,
        # hash+field forward and render (npr, M / B set per entry below)
        grid=_grid(), x=FAKE, table=FAKE, table_dtype=L.F16, planes=FAKE, plane_stride=None,
        z=FAKE, color_surf=FAKE, z_scale=1.0, numerics=L.RENDER_REFERENCE, cmap=FAKE, atmo=FAKE,
        surf=FAKE,
    )


def _b(d):
    return ctypes.byref(d)


def _fwd(name):
    def f(lib, p):
        rows = (p["rows"],) if name.endswith("_rows") else ()
        return getattr(lib, name)(_b(p["pos"]), _b(p["dir"]), p["mma"], p["packed"], p["enc"],
                                  p["enc_stride"], p["dirs"], p["npr"], p["M"], *rows,
                                  p["sigma"], p["color"], p["color_stride"], None)
    return f


def _bwd(name):
    def f(lib, p):
        rows = (p["rows"],) if name.endswith("_rows") else ()
        return getattr(lib, name)(_b(p["pos"]), _b(p["dir"]), p["mma"], p["packed"], p["enc"],
                                  p["enc_stride"], p["dirs"], p["npr"], p["M"], *rows,
                                  p["d_sigma"], p["d_color"], p["d_color_stride"], p["d_enc"],
                                  p["d_enc_stride"], p["g_pos"], p["g_dir"], p["ws"],
                                  p["ws_bytes"], None)
    return f


def _ref16(name):
    def f(lib, p):
        tail = {"anr_ingp_field_bwd_ref16": (),
                "anr_ingp_field_bwd_ref16_tiles": (p["tile_nz"],)}.get(
                    name, (p["row_nz"], p["ws"], p["ws_bytes"]))
        return getattr(lib, name)(_b(p["pos"]), _b(p["dir"]), p["packed"], p["enc"],
                                  p["enc_stride"], p["dirs"], p["npr"], p["M"], p["d_sigma"],
                                  p["d_color"], p["d_color_stride"], p["d_enc"],
                                  p["d_enc_stride"], p["g_pos"], p["g_dir"], p["loss_scale"],
                                  *tail, None)
    return f


def _density(lib, p):
    return lib.anr_ingp_field_density(_b(p["pos"]), _b(p["dir"]), p["mma"], p["packed"], p["enc"],
                                      p["enc_stride"], p["M"], p["sigma"], None)


def _pack(lib, p):
    return lib.anr_ingp_field_pack(_b(p["pos"]), _b(p["dir"]), p["mma"], p["pos_params"],
                                   p["dir_params"], p["packed"], None)


def _hash_field(lib, p):
    npr = 64 if p["npr"] == 1 else p["npr"]
    ps = 8 * max(p["M"], 1) if p["plane_stride"] is None else p["plane_stride"]
    return lib.anr_ingp_hash_field_fwd(_b(p["grid"]), p["x"], p["M"], p["table"],
                                       p["table_dtype"], p["planes"], ps, _b(p["pos"]),
                                       _b(p["dir"]), p["mma"], p["packed"], p["dirs"], npr,
                                       p["sigma"], p["color"], p["color_stride"], None)


def _render(lib, p):  # M is B here
    npr = 64 if p["npr"] == 1 else p["npr"]
    return lib.anr_ingp_render(_b(p["grid"]), p["x"], p["z"], p["dirs"], p["M"], npr, p["table"],
                               p["table_dtype"], _b(p["pos"]), _b(p["dir"]), p["mma"],
                               p["packed"], p["color_surf"], p["z_scale"], p["numerics"],
                               p["cmap"], p["atmo"], p["surf"], None)


ENTRY = {
    "fwd": _fwd("anr_ingp_field_fwd"),
    "fwd_h": _fwd("anr_ingp_field_fwd_h"),
    "fwd_rows": _fwd("anr_ingp_field_fwd_rows"),
    "density": _density,
    "bwd": _bwd("anr_ingp_field_bwd"),
    "bwd_rows": _bwd("anr_ingp_field_bwd_rows"),
    "ref16": _ref16("anr_ingp_field_bwd_ref16"),
    "ref16_tiles": _ref16("anr_ingp_field_bwd_ref16_tiles"),
    "ref16_rows": _ref16("anr_ingp_field_bwd_ref16_rows"),
    "ref16_rows_h": _ref16("anr_ingp_field_bwd_ref16_rows_h"),
    "pack": _pack,
    "hash_field": _hash_field,
    "render": _render,
}
FWD = ("fwd", "fwd_h", "fwd_rows")
BWD = ("bwd", "bwd_rows", "ref16", "ref16_tiles", "ref16_rows", "ref16_rows_h")
REF16 = BWD[2:]
ROWS16 = ("ref16_rows", "ref16_rows_h")
HF = ("hash_field", "render")
FULL = {"ref16": "anr_ingp_field_bwd_ref16:", "ref16_tiles": "anr_ingp_field_bwd_ref16_tiles:",
        "ref16_rows": "anr_ingp_field_bwd_ref16_rows:",
        "ref16_rows_h": "anr_ingp_field_bwd_ref16_rows_h:"}
# the shared bodies answer under these names
BODY = {**{e: "anr_ingp_field_fwd:" for e in FWD}, **{e: "anr_ingp_field_bwd:" for e in BWD},
        "density": "anr_ingp_field_density:", "pack": "anr_ingp_field_pack:",
        "hash_field": "anr_ingp_hash_field_fwd:", "render": "anr_ingp_render:"}


def _run(entry, **over):
    L = _lib()
    lib = L.load()
    p = _defaults()
    for k, v in over.items():
        if k not in p:
            raise KeyError(k)
        p[k] = v
    rc = ENTRY[entry](lib, p)
    return rc, lib.anr_last_error().decode()


def _refused(entry, rc, *words, **over):
    got, msg = _run(entry, **over)
    assert got == rc, (entry, over, got, msg)
    for w in words:
        assert w in msg, (entry, over, msg)


# ------------------------------------------------------------------ queries
def test_queries_answer_without_a_device():
    L = _lib()
    lib = L.load()
    pos, dird = _pair()
    bad = _pair(dir_width=32)
    assert lib.anr_ingp_field_supported(_b(pos), _b(dird)) == 1
    assert lib.anr_ingp_field_supported(_b(bad[0]), _b(bad[1])) == 0
    assert lib.anr_ingp_field_supported(None, _b(dird)) == 0
    assert lib.anr_ingp_field_packed_size(_b(bad[0]), _b(bad[1])) == 0
    sizes = {(w, n): lib.anr_ingp_field_packed_size(*map(_b, _pair(width=w, nhd=n)))
             for w in (32, 64) for n in (1, 2)}
    assert all(s > 0 for s in sizes.values()) and len(set(sizes.values())) == 4, sizes
    # the size does not depend on the density outputs
    for S in (2, 3, 4):
        assert lib.anr_ingp_field_packed_size(*map(_b, _pair(S=S))) == sizes[(64, 2)]
    ws = lib.anr_ingp_field_bwd_workspace_bytes
    assert ws(_b(bad[0]), _b(bad[1]), L.F16, 4096) == 0
    assert ws(_b(pos), _b(dird), L.BF16, 4096) == 0
    for S in (1, 2, 3, 4):
        p, d = _pair(S=S)
        assert ws(_b(p), _b(d), L.F16, 0) == 0
        assert ws(_b(p), _b(d), L.F16, -5) == 0
    rws = lib.anr_ingp_field_bwd_ref16_rows_workspace_bytes
    assert [rws(m) for m in (-1, 0, 1, 32, 33, 4096)] == [0, 0, 260, 260, 264, 256 + 4 * 128]


# ------------------------------------------------------------------ pair, dtype, M
@pytest.mark.parametrize("entry", list(ENTRY))
def test_unsupported_pair(entry):
    pos, dird = _pair(dir_width=32)  # widths differ: variant 0
    if entry in HF:
        _refused(entry, UNSUPPORTED, BODY[entry], "unsupported configuration", pos=pos, dir=dird)
    else:
        _refused(entry, INVALID, BODY[entry], "unsupported pos/dir MLP pair", pos=pos, dir=dird)


@pytest.mark.parametrize("entry", FWD + ("density", "bwd", "bwd_rows"))
def test_unsupported_pair_comes_before_empty(entry):
    pos, dird = _pair(dir_width=32)
    _refused(entry, INVALID, BODY[entry], "unsupported pos/dir MLP pair", pos=pos, dir=dird, M=0)


@pytest.mark.parametrize("mma", [0, 7])
@pytest.mark.parametrize("entry", FWD + ("density", "bwd", "bwd_rows", "pack") + HF)
def test_bad_mma_dtype(entry, mma):
    if entry in HF:
        _refused(entry, UNSUPPORTED, BODY[entry], "unsupported configuration", mma=mma)
    else:
        _refused(entry, INVALID, BODY[entry], "mma_dtype must be ANR_F16 or ANR_BF16", mma=mma)


@pytest.mark.parametrize("M", [-1, 1 << 31])
@pytest.mark.parametrize("entry", FWD + ("density",) + BWD)
def test_bad_M(entry, M):
    _refused(entry, INVALID, BODY[entry], "bad M", M=M)


def test_bad_M_hash_field_and_render():
    _refused("hash_field", INVALID, "anr_ingp_hash_field_fwd: bad M / plane_stride", M=-1)
    _refused("render", INVALID, "anr_ingp_render: bad B", M=-1)


@pytest.mark.parametrize("entry", [e for e in ENTRY if e != "pack"])
def test_empty_is_ok(entry):
    """M = 0 (B = 0) returns ANR_OK with no pointer looked at -- except the three entries
    that check their own extra pointers first (below). The pack has no M."""
    null = dict(packed=None, enc=None, dirs=None, sigma=None, color=None, d_sigma=None,
                d_color=None, d_enc=None, g_pos=None, g_dir=None, ws=None, ws_bytes=0, rows=None,
                x=None, table=None, planes=None, z=None, cmap=None)
    if entry in ("ref16_tiles",) + ROWS16:
        null.update(d_enc=FAKE, tile_nz=FAKE, row_nz=FAKE)
    rc, msg = _run(entry, M=0, **null)
    assert rc == OK, (entry, msg)
    for S in (2, 4):  # the refusal of bands does not apply to an empty call
        pos, dird = _pair(S=S)
        rc, msg = _run(entry, M=0, pos=pos, dir=dird, **null)
        assert rc == OK, (entry, S, msg)


def test_empty_hash_field_skips_every_check():
    pos, dird = _pair(dir_width=32)
    rc, _ = _run("hash_field", M=0, pos=pos, dir=dird, x=None, table_dtype=0)
    assert rc == OK


def test_own_pointers_come_before_empty():
    """_ref16_tiles, _ref16_rows and _ref16_rows_h look at loss_scale and their own
    pointers before M, for one density output and for several."""
    for S in (1, 4):
        pos, dird = _pair(S=S)
        kw = dict(M=0, pos=pos, dir=dird)
        _refused("ref16_tiles", INVALID, FULL["ref16_tiles"], "null tile_nz", tile_nz=None, **kw)
        for e in ROWS16:
            _refused(e, INVALID, FULL[e], "null d_enc / row_nz", row_nz=None, **kw)
            _refused(e, INVALID, FULL[e], "null d_enc / row_nz", d_enc=None, **kw)
            _refused(e, INVALID, FULL[e], "256-byte aligned", ws=FAKE + 128, **kw)
        for e in REF16:
            _refused(e, INVALID, FULL[e], "loss_scale must be > 0", loss_scale=0.0, **kw)


# ------------------------------------------------------------------ pointers
@pytest.mark.parametrize("entry,field", [
    *[(e, f) for e in FWD for f in ("packed", "enc", "dirs", "sigma", "color")],
    *[("density", f) for f in ("packed", "enc", "sigma")],
    *[(e, f) for e in ("bwd", "bwd_rows", "ref16", "ref16_tiles")
      for f in ("packed", "enc", "dirs", "d_color", "d_enc", "g_pos", "g_dir")],
    *[(e, f) for e in ROWS16 for f in ("packed", "enc", "dirs", "d_color", "g_pos", "g_dir")],
    *[("pack", f) for f in ("pos_params", "dir_params", "packed")],
    *[("hash_field", f) for f in ("x", "table", "planes", "packed", "dirs", "sigma", "color")],
    *[("render", f) for f in ("x", "z", "dirs", "table", "packed", "cmap")],
])
def test_null_required_pointer(entry, field):
    _refused(entry, INVALID, BODY[entry], "null pointer", **{field: None})


def test_null_pointers_of_one_entry():
    _refused("fwd_rows", INVALID, "anr_ingp_field_fwd_rows: null rows", rows=None)
    _refused("bwd_rows", INVALID, "anr_ingp_field_bwd_rows: null rows", rows=None)
    _refused("ref16_tiles", INVALID, FULL["ref16_tiles"], "null tile_nz", tile_nz=None)
    for e in ROWS16:
        _refused(e, INVALID, FULL[e], "null d_enc / row_nz", row_nz=None)
        # f16 rows (and, for _rows_h, f16 gradients) without the f16 row buffer
        _refused(e, INVALID, FULL[e], "null d_enc / row_nz", d_enc=None)


@pytest.mark.parametrize("entry,field,off,words", [
    *[(e, f, 8, ("anr_ingp_field_fwd:", "enc/packed must be 16-byte aligned"))
      for e in FWD for f in ("enc", "packed")],
    *[("density", f, 8, ("anr_ingp_field_density:", "enc/packed must be 16-byte aligned"))
      for f in ("enc", "packed")],
    *[(e, f, 8, ("anr_ingp_field_bwd:", "enc/packed/d_enc must be 16-byte aligned"))
      for e in BWD for f in ("enc", "packed")],
    *[(e, "d_enc", 8, ("anr_ingp_field_bwd:", "enc/packed/d_enc must be 16-byte aligned"))
      for e in ("bwd", "bwd_rows", "ref16", "ref16_tiles")],
    *[(e, "d_enc", 4, ("anr_ingp_field_bwd:", "(f16 rows: 8)")) for e in ROWS16],
    ("ref16_rows_h", "d_color", 4, ("anr_ingp_field_bwd:", "f16 d_color must be 8-byte aligned")),
    ("fwd_h", "color", 4, ("anr_ingp_field_fwd_h:", "color must be 8-byte aligned")),
    *[("hash_field", f, 8, ("anr_ingp_hash_field_fwd:", "must be 16-byte aligned"))
      for f in ("planes", "packed", "color")],
])
def test_misaligned_pointer(entry, field, off, words):
    _refused(entry, INVALID, *words, **{field: FAKE + off})


def test_misaligned_packed_render():
    _refused("render", UNSUPPORTED, "anr_ingp_render:", "packed weights must be 16-byte aligned",
             packed=FAKE + 8)


# ------------------------------------------------------------------ strides and shapes
@pytest.mark.parametrize("stride", [31, 36, -8, -(8 * M0 - 8), -(8 * M0 + 4)])
@pytest.mark.parametrize("entry", FWD + ("density",) + BWD)
def test_enc_stride_in_neither_form(entry, stride):
    name = "anr_ingp_field_density: bad enc_stride" if entry == "density" else \
        "anr_ingp_field: bad enc_stride %d" % stride
    _refused(entry, INVALID, name, enc_stride=stride)


@pytest.mark.parametrize("stride", [28, 34])
@pytest.mark.parametrize("entry", BWD)
def test_d_enc_stride(entry, stride):
    _refused(entry, INVALID, "anr_ingp_field_bwd: bad shape/stride", d_enc_stride=stride)


def test_colour_stride_below_outputs_and_rays():
    for e in FWD:
        _refused(e, INVALID, "anr_ingp_field_fwd: bad shape/stride", color_stride=3)
        _refused(e, INVALID, "anr_ingp_field_fwd: bad shape/stride", npr=0)
        _refused(e, INVALID, "anr_ingp_field_fwd: bad shape/stride", npr=1 << 31)
    for e in BWD:
        _refused(e, INVALID, "anr_ingp_field_bwd: bad shape/stride", d_color_stride=3)
        _refused(e, INVALID, "anr_ingp_field_bwd: bad shape/stride", npr=0)
    pos, dird = _pair(n_out=7)
    _refused("fwd", INVALID, "anr_ingp_field_fwd: bad shape/stride", pos=pos, dir=dird,
             color_stride=6)
    _refused("bwd", INVALID, "anr_ingp_field_bwd: bad shape/stride", pos=pos, dir=dird,
             d_color_stride=6)


# ------------------------------------------------------------------ reference numerics
@pytest.mark.parametrize("loss_scale", [0.0, -1.0])
@pytest.mark.parametrize("entry", REF16)
def test_loss_scale_must_be_positive(entry, loss_scale):
    _refused(entry, INVALID, FULL[entry], "loss_scale must be > 0", loss_scale=loss_scale)


@pytest.mark.parametrize("entry", ROWS16)
def test_rows_workspace(entry):
    L = _lib()
    need = L.load().anr_ingp_field_bwd_ref16_rows_workspace_bytes(M0)
    assert need == 256 + 4 * 2
    _refused(entry, INVALID, FULL[entry], "workspace smaller than", ws_bytes=need - 1)
    _refused(entry, INVALID, FULL[entry], "256-byte aligned", ws=FAKE + 128)
    _refused(entry, INVALID, FULL[entry], "256-byte aligned", ws=FAKE + 16, ws_bytes=need)
    # the size comes first
    _refused(entry, INVALID, FULL[entry], "workspace smaller than", ws=FAKE + 128, ws_bytes=0)


# ------------------------------------------------------------------ density outputs
@pytest.mark.parametrize("S,off,align", [(2, 4, 8), (4, 4, 16), (4, 8, 16), (3, 2, 4)])
def test_band_pointers_alignment(S, off, align):
    """S densities of a row leave (arrive) as one access: 4 S bytes, 4 for S = 3."""
    pos, dird = _pair(S=S)
    kw = dict(pos=pos, dir=dird)
    _refused("fwd", INVALID, "anr_ingp_field_fwd: sigma (M, %d) must be %d-byte aligned"
             % (S, align), sigma=FAKE + off, **kw)
    _refused("density", INVALID, "anr_ingp_field_density: sigma (M, %d) must be %d-byte aligned"
             % (S, align), sigma=FAKE + off, **kw)
    _refused("bwd", INVALID, "anr_ingp_field_bwd: d_sigma (M, %d) must be %d-byte aligned"
             % (S, align), d_sigma=FAKE + off, **kw)


@pytest.mark.parametrize("S", [2, 3, 4])
@pytest.mark.parametrize("entry", ("fwd_h", "fwd_rows", "bwd_rows") + REF16 + HF)
def test_bands_refused(entry, S):
    """Before any pointer: every one of them is null here."""
    pos, dird = _pair(S=S)
    name = {"fwd_h": "anr_ingp_field_fwd_h:", "fwd_rows": "anr_ingp_field_fwd_rows:",
            "bwd_rows": "anr_ingp_field_bwd_rows:", **FULL, "hash_field": BODY["hash_field"],
            "render": BODY["render"]}[entry]
    null = dict(packed=None, enc=None, dirs=None, sigma=None, color=None, d_sigma=None,
                d_color=None, d_enc=None, g_pos=None, g_dir=None, ws=None, ws_bytes=0, rows=None,
                tile_nz=None, row_nz=None, planes=None)
    if entry == "render":  # its null and numerics checks come first
        null = {}
    _refused(entry, UNSUPPORTED, name, "more than one density output", pos=pos, dir=dird, **null)


def test_band_pairs_pass_the_shared_checks():
    """An S > 1 pair is a supported pair: the entries that take it answer the next check."""
    pos, dird = _pair(S=3)
    _refused("fwd", INVALID, "anr_ingp_field_fwd: null pointer", pos=pos, dir=dird, color=None)
    _refused("density", INVALID, "anr_ingp_field_density: null pointer", pos=pos, dir=dird,
             sigma=None)
    _refused("bwd", INVALID, "anr_ingp_field_bwd: null pointer", pos=pos, dir=dird, g_dir=None)
    _refused("pack", INVALID, "anr_ingp_field_pack: null pointer", pos=pos, dir=dird, packed=None)


# ------------------------------------------------------------------ hash+field forward, render
def _hf_configs():
    pos, dird = _pair(n_out=3)
    return {
        "dims2": dict(grid=_grid(n_dims=2)), "dims4": dict(grid=_grid(n_dims=4)),
        "features": dict(grid=_grid(n_features=4)), "levels": dict(grid=_grid(n_levels=8)),
        "n_output": dict(pos=pos, dir=dird), "npr0": dict(npr=0), "npr63": dict(npr=63),
        "npr65": dict(npr=65), "table_dtype": dict(table_dtype=_lib().F32),
    }


@pytest.mark.parametrize("case", ["dims2", "dims4", "features", "levels", "n_output", "npr0",
                                  "npr63", "npr65", "table_dtype"])
@pytest.mark.parametrize("entry", HF)
def test_hash_field_unsupported_configuration(entry, case):
    _refused(entry, UNSUPPORTED, BODY[entry], "unsupported configuration", **_hf_configs()[case])


def test_hash_field_own_checks():
    for cs in (3, 6):
        _refused("hash_field", UNSUPPORTED, BODY["hash_field"], "unsupported configuration",
                 color_stride=cs)
    for ps in (8 * M0 - 8, 8 * M0 + 4):
        _refused("hash_field", INVALID, "anr_ingp_hash_field_fwd: bad M / plane_stride",
                 plane_stride=ps)
    _refused("render", INVALID, "anr_ingp_render: numerics must be", numerics=2)
    blank = _lib().HashGridDesc()
    blank.n_dims, blank.n_levels, blank.n_features = 3, 16, 2
    for e in HF:
        _refused(e, INVALID, BODY[e], "descriptor not initialised", grid=blank)


def test_byte_ranges_below_2_31():
    """Each at the first value that trips it (plane_stride = 8 M, colour rows of 4)."""
    hf = ("anr_ingp_hash_field_fwd:", "byte ranges must stay below 2^31")
    # the planes' (3 P + 8 M) * 2 bytes = 64 M reach 2^31 first
    _refused("hash_field", INVALID, *hf, M=1 << 25)
    # M * color_stride * 4
    _refused("hash_field", INVALID, *hf, color_stride=1 << 23)
    # a plane of 2^31 bytes
    _refused("hash_field", INVALID, *hf, plane_stride=1 << 30)
    rn = ("anr_ingp_render:", "byte ranges must stay below 2^31")
    # (B * 64 + 64) * 12 >= 2^31 from B = 2796202 on
    assert (2796201 * 64 + 64) * 12 < 1 << 31 <= (2796202 * 64 + 64) * 12
    _refused("render", UNSUPPORTED, *rn, M=2796202)
    _refused("render", UNSUPPORTED, *rn, M=1 << 25)  # B * n_per_ray = 2^31
    _refused("render", UNSUPPORTED, *rn, M=1, npr=1 << 31)
    # a table of 2^31 bytes: the last level ends at entry 2^29 or later
    g = _grid()
    g.offsets[16] = g.offsets[15] + (1 << 29)
    _refused("hash_field", INVALID, *hf, grid=g)
    _refused("render", UNSUPPORTED, *rn, grid=g)
