"""GPU: geosrad_sw_driver_chou_na_dev / geosrad_sw_driver_chou_na_lit_dev, the Chou-Suarez branch of SORADCORE with the aerosol-free
internals FSWNAN, FSCNAN, FSWUNAN, FSCUNAN, FSWBANDNAN from one k_swc_prep and one shared solver call, where the GridComp runs SORADCORE
a second time with include_aerosols = .false. (GEOS_SolarGridComp.F90:3249-3259, :3997-4016).  The yardstick is the existing driver
called with TAUA = SSAA = ASYA = NULL, bit for bit; outputs start poisoned (-7)."""
import ctypes

import numpy as np
import pytest

from geosradiation_gridcomp_amd import gridcomp as G
from geosradiation_gridcomp_amd import synth
from geosradiation_gridcomp_amd.api import GeosradError

pytestmark = pytest.mark.gpu
POISON = -7.0
LM = 33
TWIN = dict(zip(G.SWCNA_OUT, ("FSW", "FSC", "FSWU", "FSCU", "FSWBAND")))
SLOT_PREP, SLOT_PASS = 12, 13
AER = ("TAUA", "SSAA", "ASYA")
PREC = {4: "r4", 8: "r8"}


def rows(k):
    k = TWIN.get(k, k)
    return LM + 1 if k in ("FSW", "FSC", "FSWU", "FSCU") else (8 if k in ("FSWBAND", "DRBAND", "DFBAND") else 1)


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def launches(ctx, slot):
    ms = ctypes.c_double(); n = ctypes.c_long()
    ctx._chk(ctx.L.geosrad_profile_read(ctx.h, ctypes.c_int(slot), ctypes.byref(ms), ctypes.byref(n)))
    return n.value


@pytest.fixture(scope="module")
def fields():
    """GEOS fields as the existing Chou driver tests build theirs: 300 columns (two 256-column blocks, the second ragged) x 33 layers"""
    inp = synth.make_columns(300, LM, start=8080, cloudy_frac=0.6, aerosol=True)
    return synth.geos_chou_sw_fields(inp, aerosol=True)


@pytest.fixture(scope="module")
def tile():
    """700-column tile, about half of it lit (column 0 dark, the last one lit, one column with ZTH == 0)"""
    n = 700
    inp = synth.make_columns(n, LM, start=47_000, cloudy_frac=0.6, aerosol=True)
    f = synth.geos_chou_sw_fields(inp, aerosol=True)
    rng = np.random.default_rng(12)
    day = rng.uniform(size=n) < 0.47
    day[0] = False; day[n - 1] = True; day[300] = False
    zth = np.where(day, f["ZT"], -rng.uniform(0.01, 1.0, n))
    zth[300] = 0.0
    f["ZT"] = zth.copy()
    return f, day


def packed_call(ctx, f, ncol, na=None, aer=True, drf=True, counts=None, cols=None):
    """sw_driver_chou_dev (na None) or sw_driver_chou_na_dev (na = names of SWCNA_OUT given; "null" = na_out NULL) on the columns `cols` of
    the fields; returns (out, na_out) as numpy, poison where nothing was written"""
    import torch
    dt = ctx.dtype
    tdt = torch.float32 if dt == np.float32 else torch.float64
    sel = (lambda a: a) if cols is None else (lambda a: a[..., cols])
    t = {k: torch.from_numpy(np.ascontiguousarray(sel(np.asarray(f[k])), dtype=dt)).cuda() for k in G.SWC_IN if aer or k not in AER}
    out = {k: torch.full((rows(k), ncol), POISON, dtype=tdt, device="cuda") for k in G.SWC_OUT}
    nao = {k: torch.full((rows(k), ncol), POISON, dtype=tdt, device="cuda") for k in G.SWCNA_OUT}
    ptr = {k: v.data_ptr() for k, v in {**t, **out}.items()}
    tail = (G.swc_consts(co2=f["CO2"]), f["LCLDMH"], f["LCLDLM"], f["HK_UV"], f["HK_IR"])
    if counts is not None:
        ctx.profile(True)
    try:
        if na is None:
            ctx.sw_driver_chou_dev(_stream(), ncol, LM, ptr, *tail, do_drfband=drf)
        else:
            ctx.sw_driver_chou_na_dev(_stream(), ncol, LM, ptr, *tail, do_drfband=drf,
                                      na_ptr=None if na == "null" else {k: nao[k].data_ptr() for k in na})
        ctx.check(_stream())
        if counts is not None:
            counts["prep"] = launches(ctx, SLOT_PREP); counts["pass"] = launches(ctx, SLOT_PASS)
    finally:
        if counts is not None:
            ctx.profile(False)
    return {k: v.cpu().numpy() for k, v in out.items()}, {k: v.cpu().numpy() for k, v in nao.items()}


@pytest.mark.parametrize("rk", [4, 8])
def test_packed_driver(gpu_ctx, fields, rk):
    ctx = gpu_ctx[rk]
    n = 300
    cp, cn, cz = {}, {}, {}
    w, wn = packed_call(ctx, fields, n, counts=cp)                               # the plain driver with aerosols ...
    z, _ = packed_call(ctx, fields, n, aer=False)                                # ... and with TAUA = SSAA = ASYA = NULL
    g, gn = packed_call(ctx, fields, n, na=G.SWCNA_OUT, counts=cn)
    for k in G.SWC_OUT:
        assert np.array_equal(g[k], w[k]), k
        assert np.isfinite(g[k]).all() and (g[k] != POISON).all(), k
    for k in G.SWCNA_OUT:
        assert np.array_equal(gn[k], z[TWIN[k]]), k
        assert (wn[k] == POISON).all(), k
    assert not np.array_equal(gn["FSWNA"], g["FSW"])
    assert cn["prep"] == cp["prep"] and cn["pass"] == 2 * cp["pass"], (cp, cn)
    # no aerosols to take away: no second pass, the aerosol-free outputs are their twins
    h, hn = packed_call(ctx, fields, n, na=G.SWCNA_OUT, aer=False, counts=cz)
    assert cz == cp, (cz, cp)
    for k in G.SWC_OUT:
        assert np.array_equal(h[k], z[k]), k
    for k in G.SWCNA_OUT:
        assert np.array_equal(hn[k], h[TWIN[k]]), k
    # members not given are left untouched, with and without aerosol inputs; na_out NULL is the plain driver
    for aer in (True, False):
        s, sn = packed_call(ctx, fields, n, na=("FSCNA", "FSWBANDNA"), aer=aer, drf=False)
        for k in G.SWCNA_OUT:
            if k in ("FSCNA", "FSWBANDNA"):
                assert np.array_equal(sn[k], gn[k]), (aer, k)
            else:
                assert (sn[k] == POISON).all(), (aer, k)
        assert (s["DRBAND"] == POISON).all() and (s["DFBAND"] == POISON).all()      # do_drfband keeps its meaning
        assert np.array_equal(s["FSW"], (w if aer else z)["FSW"])
    c0 = {}
    p, pn = packed_call(ctx, fields, n, na="null", counts=c0)
    assert c0 == cp and all(np.array_equal(p[k], w[k]) for k in G.SWC_OUT) and all((pn[k] == POISON).all() for k in G.SWCNA_OUT)


def dark_values():
    """a DEFAULT of its own for every output, exactly representable in fp32"""
    return {k: -100.0 - 0.5 * i for i, k in enumerate(G.SWC_OUT)}, {k: -200.0 - 0.5 * i for i, k in enumerate(G.SWCNA_OUT)}


def tile_call(ctx, f, zth, na=G.SWCNA_OUT, keep=("FSWU",), keep_na=("FSCUNA",), dark_na="default", plain=False):
    """the lit index of the tile, then sw_driver_chou_na_lit_dev (or sw_driver_chou_lit_dev) on poisoned tile-wide outputs"""
    import torch
    n = zth.size
    dt = ctx.dtype
    tdt = torch.float32 if dt == np.float32 else torch.float64
    t = {k: torch.from_numpy(np.ascontiguousarray(f[k], dtype=dt)).cuda() for k in G.SWC_IN}
    z = torch.from_numpy(np.ascontiguousarray(zth, dtype=dt)).cuda()
    idx = torch.full((n,), -9, dtype=torch.int32, device="cuda"); pos = torch.full((n,), -9, dtype=torch.int32, device="cuda")
    nl = torch.zeros(1, dtype=torch.int32, device="cuda")
    nlit = ctx.lit_index_dev(_stream(), n, z.data_ptr(), idx.data_ptr(), pos.data_ptr(), nl.data_ptr())
    out = {k: torch.full((rows(k), n), POISON, dtype=tdt, device="cuda") for k in G.SWC_OUT}
    nao = {k: torch.full((rows(k), n), POISON, dtype=tdt, device="cuda") for k in G.SWCNA_OUT}
    ptr = {k: v.data_ptr() for k, v in {**t, **out}.items()}
    d, dn = dark_values()
    args = (_stream(), n, nlit, idx.data_ptr(), pos.data_ptr(), LM, ptr, G.swc_consts(co2=f["CO2"]), f["LCLDMH"], f["LCLDLM"], f["HK_UV"], f["HK_IR"])
    if plain:
        ctx.sw_driver_chou_lit_dev(*args, do_drfband=True, dark=d, keep=keep)
    else:
        ctx.sw_driver_chou_na_lit_dev(*args, do_drfband=True, dark=d, keep=keep, na_ptr={k: nao[k].data_ptr() for k in na},
                                      dark_na=dn if dark_na == "default" else dark_na, keep_na=keep_na)
    ctx.check(_stream())
    return nlit, idx.cpu().numpy(), {k: v.cpu().numpy() for k, v in out.items()}, {k: v.cpu().numpy() for k, v in nao.items()}


@pytest.mark.parametrize("rk", [4, 8])
def test_tile(gpu_ctx, tile, rk):
    ctx = gpu_ctx[rk]
    f, day = tile
    n = day.size
    d, dn = dark_values()
    nlit, idx, b, bn = tile_call(ctx, f, f["ZT"])
    assert nlit == int(day.sum()) and 0.4 * n < nlit < 0.6 * n
    assert np.array_equal(idx[:nlit], np.where(day)[0])
    _, _, p, _ = tile_call(ctx, f, f["ZT"], plain=True)
    for k in G.SWC_OUT:
        assert np.array_equal(b[k], p[k]), k                                   # out is bitwise sw_driver_chou_lit_dev
    # lit columns: the packed driver on the gathered columns, scattered
    g, gn = packed_call(ctx, f, nlit, na=G.SWCNA_OUT, cols=np.where(day)[0])
    for k in G.SWCNA_OUT:
        assert np.array_equal(bn[k][:, day], gn[k]), k
        want = POISON if k == "FSCUNA" else dn[k]                                # the kept one keeps its old value
        assert (bn[k][:, ~day] == np.asarray(want, dtype=ctx.dtype)).all(), k
    for k in G.SWC_OUT:
        assert np.array_equal(b[k][:, day], g[k]), k
        assert (b[k][:, ~day] == np.asarray(POISON if k == "FSWU" else d[k], dtype=ctx.dtype)).all(), k
    assert not np.array_equal(bn["FSWNA"][:, day], b["FSW"][:, day])
    # a member not given stays untouched on lit and dark columns alike
    _, _, _, sn = tile_call(ctx, f, f["ZT"], na=("FSWNA",))
    assert np.array_equal(sn["FSWNA"], bn["FSWNA"]) and all((sn[k] == POISON).all() for k in G.SWCNA_OUT if k != "FSWNA")
    # no lit column: only the dark values are written
    night = -np.abs(f["ZT"]) - 0.01
    counts = {}
    ctx.profile(True)
    try:
        nl0, _, a, an = tile_call(ctx, dict(f, ZT=night), night)
        counts = {"prep": launches(ctx, SLOT_PREP), "pass": launches(ctx, SLOT_PASS)}
    finally:
        ctx.profile(False)
    assert nl0 == 0 and counts == {"prep": 0, "pass": 0}
    for k in G.SWCNA_OUT:
        assert (an[k] == np.asarray(POISON if k == "FSCUNA" else dn[k], dtype=ctx.dtype)).all(), k
    for k in G.SWC_OUT:
        assert (a[k] == np.asarray(POISON if k == "FSWU" else d[k], dtype=ctx.dtype)).all(), k
    # dark_na NULL while a requested aerosol-free output has its keep bit clear: refused, nothing written
    with pytest.raises(GeosradError) as e:
        tile_call(ctx, f, f["ZT"], dark_na=None)
    assert e.value.rc == 1
    # ... and accepted when every requested one is kept
    _, _, _, kn = tile_call(ctx, f, f["ZT"], dark_na=None, keep_na=G.SWCNA_OUT)
    for k in G.SWCNA_OUT:
        assert np.array_equal(kn[k][:, day], gn[k]) and (kn[k][:, ~day] == POISON).all(), k


@pytest.mark.parametrize("rk", [4, 8])
def test_downstream_exports_and_heating_rates(gpu_ctx, fields, rk):
    """The driver's out and na_out as the internals FSWN ... FSWBANDNAN of UPDATE_EXPORT (FSWNA, RSRNA, OSRNA) and, through its exports,
    of the parent's heating rates (RADSWNA).  The yardstick is the plain-C oracle (clib.sw_update_export, clib.rad_tendencies), not numpy
    expressions: it is what tests/test_gpu_gridcomp.py holds the with-aerosol twins to, bit for bit."""
    import torch
    from oracle import clib
    ctx = gpu_ctx[rk]; dt = ctx.dtype
    tdt = torch.float32 if rk == 4 else torch.float64
    n = 300
    g, gn = packed_call(ctx, fields, n, na=G.SWCNA_OUT)
    rng = np.random.default_rng(3)
    sw = {"SLR": rng.uniform(200, 1300, n).astype(dt), "FSWN": g["FSW"], "FSCN": g["FSC"], "FSWUN": g["FSWU"], "FSCUN": g["FSCU"],
          "FSWBANDN": g["FSWBAND"], "FSWNAN": gn["FSWNA"], "FSCNAN": gn["FSCNA"], "FSWUNAN": gn["FSWUNA"], "FSCUNAN": gn["FSCUNA"],
          "FSWBANDNAN": gn["FSWBANDNA"]}
    assert set(sw) == set(G.SWU_IN)
    t = {k: torch.from_numpy(np.ascontiguousarray(v, dtype=dt)).cuda() for k, v in sw.items()}
    shp = lambda k: (LM + 1, n) if k in G.SWU_OUT_3D else ((8, n) if k in G.SWU_OUT_BAND else (n,))
    out = {k: torch.full(shp(k), POISON, dtype=tdt, device="cuda") for k in G.SWU_OUT}
    ctx.sw_update_export_dev(_stream(), n, LM, 8, {k: v.data_ptr() for k, v in {**t, **out}.items()})
    ctx.check(_stream())
    e = {k: v.cpu().numpy() for k, v in out.items()}
    o = clib.sw_update_export(sw, LM, 8, PREC[rk], want=list(G.SWU_OUT))
    undef = np.asarray(G.MAPL["UNDEF"], dtype=dt)
    for k, twin in (("FSWNA", "FSW"), ("RSRNA", "RSR"), ("OSRNA", "OSR"), ("FSCNA", "FSC"), ("FSWBANDNA", "FSWBAND")):
        assert np.array_equal(e[k], o[k]), k
        assert np.isfinite(e[k]).all() and (e[k] != undef).all() and (e[k] != POISON).all(), k
        assert not np.array_equal(e[k], e[twin]), k
    # heating rates
    rt = {k: rng.uniform(-300, 300, (LM + 1, n)).astype(dt) for k in ("FLW", "FLWCLR", "FLA")}
    rt.update(FSW=e["FSW"], FSWCLR=e["FSC"], FSWNA=e["FSWNA"], FSCNA=e["FSCNA"])
    rt["PLE"] = np.ascontiguousarray(fields["PLE"], dtype=dt)
    rt["DSFDTS"] = rng.uniform(4, 6, n).astype(dt); rt["SFCEM"] = rng.uniform(300, 450, n).astype(dt); rt["TRD"] = rng.uniform(270, 300, n).astype(dt)
    assert set(rt) == set(G.RT_IN)
    t = {k: torch.from_numpy(np.ascontiguousarray(v, dtype=dt)).cuda() for k, v in rt.items()}
    out = {k: torch.full((LM, n) if k in G.RT_OUT_3D else (n,), POISON, dtype=tdt, device="cuda") for k in G.RT_OUT}
    ctx.rad_tendencies_dev(_stream(), n, LM, G.MAPL["GRAV"], G.MAPL["CP"], {k: v.data_ptr() for k, v in {**t, **out}.items()})
    ctx.check(_stream())
    h = {k: v.cpu().numpy() for k, v in out.items()}
    o = clib.rad_tendencies(rt, LM, G.MAPL["GRAV"], G.MAPL["CP"], PREC[rk])
    for k in ("RADSWNA", "RADSWCNA", "RADSW"):
        assert np.array_equal(h[k], o[k]), k
        assert np.isfinite(h[k]).all() and (h[k] != undef).all() and (h[k] != POISON).all(), k
    assert not np.array_equal(h["RADSWNA"], h["RADSW"])
