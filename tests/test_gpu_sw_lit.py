"""GPU: geosrad_sw_driver_rrtmg_lit_dev / geosrad_sw_driver_chou_lit_dev, the SW branch of SORADCORE on the un-packed tile (PackIt of the
imports inside the prep kernels, UnPackIt with its DEFAULT inside the post kernel and one scatter: GEOS_SolarGridComp.F90:3686,
:3839-3894, :6520-6580), against the route they replace: geosrad_lit_pack_dev of every input, the packed driver on NumLit columns,
geosrad_lit_unpack_dev of every output.  Both routes hand the solver identical arrays, so every comparison is bitwise.

Tile: 700 columns (two full 256-column blocks and a ragged one) x 72 layers, lit with probability 0.47 (NumLit is no multiple of 64, so a
wavefront's index straddles), column 0 dark, the last column lit, one column with ZTH == 0 (dark)."""
import os
import numpy as np
import pytest

from geosradiation_gridcomp_amd import gridcomp as G
from geosradiation_gridcomp_amd import synth
from geosradiation_gridcomp_amd.api import GeosradError, GeosradInputError

pytestmark = pytest.mark.gpu
N, LM = 700, 72
SENTINEL = -7.0
UNDEF = G.MAPL["UNDEF"]
SWD_KEEP = ("FSC", "NIRF")          # one output of the post kernel, one of the scatter
SWC_KEEP = ("FSWU", "PARR")
SWD_ARGS = (3, 1, 1361.0, 1.0, 0)     # iceflgsw, liqflgsw, sc, dist, isolvar


def swd_rows(k):
    return LM + 1 if k in ("FSW", "FSC", "FSWU", "FSCU", "FSWNA", "FSCNA", "FSWUNA", "FSCUNA") else (14 if k.startswith("FSWBAND") else 1)


def swc_rows(k):
    return LM + 1 if k in ("FSW", "FSC", "FSWU", "FSCU") else (8 if k in ("FSWBAND", "DRBAND", "DFBAND") else 1)


def dark_of(names):
    """a DEFAULT of its own for every output, exactly representable in fp32"""
    return {k: -100.0 - 0.5 * i for i, k in enumerate(names)}


def make_zth(coszen, seed=11, all_dark=False, all_lit=False):
    rng = np.random.default_rng(seed)
    day = rng.uniform(size=N) < 0.47
    day[0] = False; day[N - 1] = True; day[300] = False
    if all_lit:
        day[:] = True
    if all_dark:
        day[:] = False
    zth = np.where(day, coszen, -rng.uniform(0.01, 1.0, N))
    if not all_lit:
        zth[300] = 0.0                  # ZTH == 0 is night (`daytime = ZTH > 0.`)
    return zth, day


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


class Tile:
    """the fields of one tile on the device, its lit index, and the two routes"""

    def __init__(self, ctx, fields, zth, in_names, out_names, rows):
        import torch
        self.ctx, self.in_names, self.out_names, self.rows = ctx, in_names, out_names, rows
        self.tdt = torch.float32 if ctx.dtype == np.float32 else torch.float64
        self.host = {k: np.ascontiguousarray(fields[k], dtype=ctx.dtype).reshape(-1, N) for k in in_names if fields.get(k) is not None}
        self.zth = torch.from_numpy(np.ascontiguousarray(zth, dtype=ctx.dtype)).cuda()
        self.idx = torch.full((N,), -9, dtype=torch.int32, device="cuda")
        self.pos = torch.full((N,), -9, dtype=torch.int32, device="cuda")
        self.nl = torch.zeros(1, dtype=torch.int32, device="cuda")
        self.nlit = ctx.lit_index_dev(_stream(), N, self.zth.data_ptr(), self.idx.data_ptr(), self.pos.data_ptr(), self.nl.data_ptr())

    def inputs(self):
        import torch
        return {k: torch.from_numpy(v).cuda() for k, v in self.host.items()}

    def outputs(self, names, width):
        import torch
        return {k: torch.full((self.rows(k), width), SENTINEL, dtype=self.tdt, device="cuda") for k in names}

    def route_a(self, names, dark, keep, call):
        """lit_pack of every input, call(nlit, ptr) = the packed driver, lit_unpack of every output"""
        import torch
        st, nlit = _stream(), self.nlit
        t = self.inputs()
        p = {k: torch.empty((v.shape[0], nlit), dtype=self.tdt, device="cuda") for k, v in t.items()}
        for k in t:
            self.ctx.lit_pack_dev(st, nlit, N, t[k].shape[0], self.idx.data_ptr(), self.nl.data_ptr(), t[k].data_ptr(), p[k].data_ptr())
        po, to = self.outputs(names, nlit), self.outputs(names, N)
        ptr = {k: v.data_ptr() for k, v in p.items()}
        ptr.update({k: v.data_ptr() for k, v in po.items()})
        call(nlit, ptr)
        for k in names:
            self.ctx.lit_unpack_dev(st, nlit, N, self.rows(k), self.pos.data_ptr(), po[k].data_ptr(), to[k].data_ptr(),
                                    default=None if k in keep else dark[k])
        self.ctx.check(st)
        return {k: v.cpu().numpy() for k, v in to.items()}

    def route_b(self, names, call):
        """call(nlit, idx, pos, ptr) = the lit-aware driver on the tile; also returns the tile's inputs as the call left them"""
        t, to = self.inputs(), self.outputs(names, N)
        ptr = {k: v.data_ptr() for k, v in t.items()}
        ptr.update({k: v.data_ptr() for k, v in to.items()})
        call(self.nlit, self.idx.data_ptr(), self.pos.data_ptr(), ptr)
        self.ctx.check(_stream())
        return {k: v.cpu().numpy() for k, v in to.items()}, {k: v.cpu().numpy() for k, v in t.items()}


# ---- RRTMG ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def swd_case():
    inp = synth.make_columns(N, LM, start=31_000, cloudy_frac=0.6, aerosol=True, distinct_albedos=True)
    f = synth.geos_sw_fields(inp)
    zth, day = make_zth(f["ZT"])
    f["ZT"] = zth.copy()
    return f, zth, day, int(inp["dyofyr"])


def swd_names(aerosols):
    return list(G.SWD_OUT) if aerosols else [k for k in G.SWD_OUT if not k.endswith("NA")]


def swd_fields(f, aerosols):
    g = dict(f)
    if not aerosols:
        g["TAUA"] = None; g["SSAA"] = None; g["ASYA"] = None
    return g


def swd_packed(ctx, f, doy, aerosols):
    return lambda nlit, ptr: ctx.sw_driver_rrtmg_dev(_stream(), nlit, LM, 14 if aerosols else 0, ptr, G.swd_consts(), *SWD_ARGS, doy, aerosols,
                                                     f["LCLDLM"], f["LCLDMH"], 1)


def swd_lit(ctx, f, doy, aerosols, dark, keep=SWD_KEEP, isolvar=0, ncol=N):
    a = SWD_ARGS[:4] + (isolvar,)
    return lambda nlit, idx, pos, ptr: ctx.sw_driver_rrtmg_lit_dev(_stream(), ncol, nlit, idx, pos, LM, 14 if aerosols else 0, ptr, G.swd_consts(),
                                                                   *a, doy, aerosols, f["LCLDLM"], f["LCLDMH"], 1, dark=dark, keep=keep)


_swd_b = {}


def swd_route_b(ctx, rk, case, aerosols):
    """route B of the module's tile under the default chunk, once per (kind, flavour)"""
    if (rk, aerosols) not in _swd_b:
        f, zth, day, doy = case
        names = swd_names(aerosols)
        tile = Tile(ctx, swd_fields(f, aerosols), zth, G.SWD_IN, names, swd_rows)
        ctx.set_inhomogeneity(1)
        try:
            _swd_b[(rk, aerosols)] = tile.route_b(names, swd_lit(ctx, f, doy, aerosols, dark_of(G.SWD_OUT)))
        finally:
            ctx.set_inhomogeneity(0)
    return _swd_b[(rk, aerosols)]


def check_dark_and_keep(got, day, names, dark, keep, dt):
    for k in names:
        if k in keep:
            assert (got[k][:, ~day] == SENTINEL).all(), k
        else:
            np.testing.assert_array_equal(got[k][:, ~day], np.full_like(got[k][:, ~day], dt(dark[k])), err_msg=k)


@pytest.mark.parametrize("aerosols", [True, False])
@pytest.mark.parametrize("rk", [4, 8])
def test_rrtmg_route_b_equals_route_a(gpu_ctx, swd_case, rk, aerosols):
    ctx = gpu_ctx[rk]
    f, zth, day, doy = swd_case
    names, dark = swd_names(aerosols), dark_of(G.SWD_OUT)
    tile = Tile(ctx, swd_fields(f, aerosols), zth, G.SWD_IN, names, swd_rows)
    assert tile.nlit == int(day.sum()) and tile.nlit % 64 != 0 and 0 < tile.nlit < N
    ctx.set_inhomogeneity(1)
    try:
        a = tile.route_a(names, dark, SWD_KEEP, swd_packed(ctx, f, doy, aerosols))
    finally:
        ctx.set_inhomogeneity(0)
    b, left = swd_route_b(ctx, rk, swd_case, aerosols)
    for k in names:
        np.testing.assert_array_equal(b[k], a[k], err_msg=k)
    check_dark_and_keep(b, day, names, dark, SWD_KEEP, ctx.dtype)
    for k in ("FSW", "FSWU", "NIRR", "FSWBAND"):
        assert not (b[k][:, day] == SENTINEL).any() and not (b[k][:, day] == ctx.dtype(dark[k])).any(), k
    if aerosols:      # the imports are read only (the reference normalises BufInp, SOL:6116-6125)
        for k in ("TAUA", "SSAA", "ASYA"):
            np.testing.assert_array_equal(left[k], tile.host[k], err_msg=k)
        assert np.abs(b["FSC"][:, day] - b["FSCNA"][:, day]).max() > 1e-3
    cot = b["COTLP"][0, day]
    assert (cot == ctx.dtype(UNDEF)).any() and (cot != ctx.dtype(UNDEF)).any()      # not an all-clear batch


@pytest.mark.parametrize("rk", [4, 8])
def test_rrtmg_small_chunk_has_the_same_bits(gpu_ctx, swd_case, rk):
    ctx = gpu_ctx[rk]
    f, zth, day, doy = swd_case
    names = swd_names(True)
    whole, _ = swd_route_b(ctx, rk, swd_case, True)
    tile = Tile(ctx, f, zth, G.SWD_IN, names, swd_rows)
    assert tile.nlit > 2 * 128 and tile.nlit % 128 != 0          # several chunks, the last ragged
    ctx.set_inhomogeneity(1); ctx.set_chunk(128)
    try:
        b, _ = tile.route_b(names, swd_lit(ctx, f, doy, True, dark_of(G.SWD_OUT)))
    finally:
        ctx.set_chunk(131072); ctx.set_inhomogeneity(0)
    for k in names:
        np.testing.assert_array_equal(b[k], whole[k], err_msg=k)


@pytest.fixture(scope="module")
def lit_bands_ctx():
    """contexts whose RRTMG_SW band sweeps are k_sw_bands (GEOSRAD_SW_PATH=bands, read when the context is created)"""
    from geosradiation_gridcomp_amd.api import Context
    old = os.environ.get("GEOSRAD_SW_PATH")
    os.environ["GEOSRAD_SW_PATH"] = "bands"
    try:
        ctxs = {4: Context(4), 8: Context(8)}
    finally:
        if old is None:
            del os.environ["GEOSRAD_SW_PATH"]
        else:
            os.environ["GEOSRAD_SW_PATH"] = old
    yield ctxs
    for c in ctxs.values():
        c.close()


@pytest.mark.parametrize("rk", [4, 8])
def test_rrtmg_route_b_equals_route_a_under_the_first_sw_mapping(lit_bands_ctx, swd_case, rk):
    ctx = lit_bands_ctx[rk]
    f, zth, day, doy = swd_case
    names, dark = swd_names(True), dark_of(G.SWD_OUT)
    tile = Tile(ctx, f, zth, G.SWD_IN, names, swd_rows)
    ctx.set_inhomogeneity(1)
    try:
        a = tile.route_a(names, dark, SWD_KEEP, swd_packed(ctx, f, doy, True))
        b, _ = tile.route_b(names, swd_lit(ctx, f, doy, True, dark))
    finally:
        ctx.set_inhomogeneity(0)
    for k in names:
        np.testing.assert_array_equal(b[k], a[k], err_msg=k)
    assert not (b["FSW"][:, day] == SENTINEL).any()


@pytest.mark.parametrize("rk", [4, 8])
def test_rrtmg_identity_index_equals_the_packed_driver(gpu_ctx, swd_case, rk):
    ctx = gpu_ctx[rk]
    f, _, _, doy = swd_case
    f = dict(f)
    zth, day = make_zth(np.clip(np.abs(f["ZT"]), 0.05, 1.0), all_lit=True)
    f["ZT"] = zth.copy()
    names = swd_names(True)
    tile = Tile(ctx, f, zth, G.SWD_IN, names, swd_rows)
    assert tile.nlit == N
    np.testing.assert_array_equal(tile.idx.cpu().numpy(), np.arange(N))
    t, to = tile.inputs(), tile.outputs(names, N)
    ptr = {k: v.data_ptr() for k, v in t.items()}
    ptr.update({k: v.data_ptr() for k, v in to.items()})
    swd_packed(ctx, f, doy, True)(N, ptr)
    ctx.check(_stream())
    b, _ = tile.route_b(names, swd_lit(ctx, f, doy, True, dark_of(G.SWD_OUT), keep=()))
    for k in names:
        np.testing.assert_array_equal(b[k], to[k].cpu().numpy(), err_msg=k)


@pytest.mark.parametrize("rk", [4, 8])
def test_rrtmg_no_lit_column(gpu_ctx, swd_case, rk):
    ctx = gpu_ctx[rk]
    f, _, _, doy = swd_case
    zth, day = make_zth(f["ZT"], all_dark=True)
    names, dark = swd_names(True), dark_of(G.SWD_OUT)
    tile = Tile(ctx, f, zth, G.SWD_IN, names, swd_rows)
    assert tile.nlit == 0 and (tile.pos.cpu().numpy() == -1).all()
    b, left = tile.route_b(names, swd_lit(ctx, f, doy, True, dark))        # returns GEOSRAD_OK; route_b runs ctx.check
    check_dark_and_keep(b, day, names, dark, SWD_KEEP, ctx.dtype)
    for k in ("TAUA", "SSAA", "ASYA"):
        np.testing.assert_array_equal(left[k], tile.host[k], err_msg=k)


# ---- Chou-Suarez ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def swc_case():
    inp = synth.make_columns(N, LM, start=47_000, cloudy_frac=0.6, aerosol=True, distinct_albedos=True)
    f = synth.geos_chou_sw_fields(inp, aerosol=True)
    zth, day = make_zth(f["ZT"], seed=12)
    f["ZT"] = zth.copy()
    return f, zth, day


@pytest.mark.parametrize("aer,drf,overcast", [(True, True, False), (False, False, False), (True, False, True)])
@pytest.mark.parametrize("rk", [4, 8])
def test_chou_route_b_equals_route_a(gpu_ctx, swc_case, rk, aer, drf, overcast):
    ctx = gpu_ctx[rk]
    f, zth, day = swc_case
    g = dict(f)
    if not aer:
        g["TAUA"] = None; g["SSAA"] = None; g["ASYA"] = None
    names = list(G.SWC_OUT) if drf else [k for k in G.SWC_OUT if k not in ("DRBAND", "DFBAND")]
    dark, consts = dark_of(G.SWC_OUT), G.swc_consts(co2=f["CO2"])
    tile = Tile(ctx, g, zth, G.SWC_IN, names, swc_rows)
    assert tile.nlit == int(day.sum()) and tile.nlit % 64 != 0
    tail = (consts, f["LCLDMH"], f["LCLDLM"], f["HK_UV"], f["HK_IR"])
    if overcast:
        ctx.set_overcast(sorad=True)
    try:
        a = tile.route_a(names, dark, SWC_KEEP, lambda nlit, ptr: ctx.sw_driver_chou_dev(_stream(), nlit, LM, ptr, *tail, do_drfband=drf))
        b, left = tile.route_b(names, lambda nlit, idx, pos, ptr: ctx.sw_driver_chou_lit_dev(_stream(), N, nlit, idx, pos, LM, ptr, *tail,
                                                                                             do_drfband=drf, dark=dark, keep=SWC_KEEP))
    finally:
        ctx.set_overcast()
    for k in names:
        np.testing.assert_array_equal(b[k], a[k], err_msg=k)
    check_dark_and_keep(b, day, names, dark, SWC_KEEP, ctx.dtype)
    assert (b["FSW"][0, day] > 0.3).all() and not (b["FSWBAND"][:, day] == SENTINEL).any()
    for k in left:
        np.testing.assert_array_equal(left[k], tile.host[k], err_msg=k)


@pytest.mark.parametrize("rk", [4, 8])
def test_chou_no_lit_column(gpu_ctx, swc_case, rk):
    ctx = gpu_ctx[rk]
    f, _, _ = swc_case
    zth, day = make_zth(f["ZT"], all_dark=True)
    names, dark = list(G.SWC_OUT), dark_of(G.SWC_OUT)
    tile = Tile(ctx, f, zth, G.SWC_IN, names, swc_rows)
    assert tile.nlit == 0
    b, _ = tile.route_b(names, lambda nlit, idx, pos, ptr: ctx.sw_driver_chou_lit_dev(
        _stream(), N, nlit, idx, pos, LM, ptr, G.swc_consts(co2=f["CO2"]), f["LCLDMH"], f["LCLDLM"], f["HK_UV"], f["HK_IR"], do_drfband=True,
        dark=dark, keep=SWC_KEEP))
    check_dark_and_keep(b, day, names, dark, SWC_KEEP, ctx.dtype)


# ---- argument errors (host-checked arguments only) -----------------------------------------------------------------------------
@pytest.mark.parametrize("rk", [4, 8])
def test_argument_errors_leave_the_outputs_alone(gpu_ctx, swd_case, swc_case, rk):
    ctx = gpu_ctx[rk]
    f, zth, day, doy = swd_case
    names, dark = swd_names(True), dark_of(G.SWD_OUT)
    tile = Tile(ctx, f, zth, G.SWD_IN, names, swd_rows)
    t, to = tile.inputs(), tile.outputs(names, N)
    ptr = {k: v.data_ptr() for k, v in t.items()}
    ptr.update({k: v.data_ptr() for k, v in to.items()})
    idx, pos, nlit = tile.idx.data_ptr(), tile.pos.data_ptr(), tile.nlit
    all_kept = tuple(names)
    cases = [
        ("nlit > ncol", dict(nlit=N + 1), GeosradError),
        ("nlit < 0", dict(nlit=-1), GeosradError),
        ("lit_index NULL", dict(idx=None), GeosradError),
        ("lit_pos NULL, an output not kept", dict(pos=None), GeosradError),
        ("lit_pos NULL, nlit > 0, all kept", dict(pos=None, keep=all_kept), GeosradError),
        ("lit_pos NULL, nlit == 0, an output not kept", dict(nlit=0, pos=None), GeosradError),
        ("dark NULL, nlit == 0, an output not kept", dict(nlit=0, dark=None), GeosradError),
        ("dark NULL, an output not kept", dict(dark=None), GeosradError),
        ("isolvar 1", dict(isolvar=1), GeosradInputError),
    ]
    for what, kw, exc in cases:
        call = swd_lit(ctx, f, doy, True, kw.get("dark", dark), keep=kw.get("keep", SWD_KEEP), isolvar=kw.get("isolvar", 0))
        with pytest.raises(exc) as e:
            call(kw.get("nlit", nlit), kw.get("idx", idx), kw.get("pos", pos), ptr)
        assert e.value.rc == (5 if exc is GeosradInputError else 1), what
        assert (exc is GeosradInputError) == isinstance(e.value, GeosradInputError), what
    ctx.check(_stream())
    for k in names:
        assert (to[k].cpu().numpy() == SENTINEL).all(), k
    # the Chou-Suarez driver
    fc, zc, _ = swc_case
    cn, cdark = list(G.SWC_OUT), dark_of(G.SWC_OUT)
    ct = Tile(ctx, fc, zc, G.SWC_IN, cn, swc_rows)
    t2, to2 = ct.inputs(), ct.outputs(cn, N)
    ptr2 = {k: v.data_ptr() for k, v in t2.items()}
    ptr2.update({k: v.data_ptr() for k, v in to2.items()})
    tail = (G.swc_consts(co2=fc["CO2"]), fc["LCLDMH"], fc["LCLDLM"], fc["HK_UV"], fc["HK_IR"])
    i2, p2 = ct.idx.data_ptr(), ct.pos.data_ptr()
    for what, a in (("nlit > ncol", (N + 1, i2, p2, cdark)), ("nlit < 0", (-1, i2, p2, cdark)), ("lit_index NULL", (ct.nlit, None, p2, cdark)),
                    ("lit_pos NULL", (ct.nlit, i2, None, cdark)), ("dark NULL", (ct.nlit, i2, p2, None)),
                    ("lit_pos NULL, nlit == 0", (0, i2, None, cdark))):
        with pytest.raises(GeosradError) as e:
            ctx.sw_driver_chou_lit_dev(_stream(), N, a[0], a[1], a[2], LM, ptr2, *tail, do_drfband=True, dark=a[3], keep=SWC_KEEP)
        assert e.value.rc == 1, what
    ctx.check(_stream())
    for k in cn:
        assert (to2[k].cpu().numpy() == SENTINEL).all(), k
