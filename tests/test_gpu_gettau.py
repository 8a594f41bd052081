"""GPU (pytest -m gpu): the batched gettau entry points of include/geosrad_gettau.h - geosrad_getvistau / getnirtau / getirtau, their `_dev`
variants and geosrad_lw_cloud_diag_dev - against the plain-C restatement of gettau.F90 (tests/gettau_impl.h, checked bit for bit against
the oracle's statement of the same routines in tests/test_gettau_oracle.py), and device against device.

Bounds.  fp64: rtol 1e-12 / atol 1e-12, the project's bound for the Chou cloud optics (tests/test_gpu_chou.py).  fp32: rtol 2e-6 for the
in-cloud thicknesses, asycl and ssacl (the same operations in the same order: only the division and the compiler's freedom remain);
rtol 2e-4 for taudiag (the device's power function against libm's powf); 7.4e-5 absolute for tcldlyr / enn (e^-1 x 2e-4: the largest
effect of that relative error on exp(-1.66 tau), times fcld <= 1).  The overlap-scaled taubeam / taudiff go through log10 and a cancelling
table interpolation: K_LOG10 = 64 eps of the species' UNSCALED thickness plus 2 ulp, the rule tests/test_sw_clouds.py derived and measured for
this arithmetic, in both precisions.  Every comparison prints its measured maximum (pytest -s); profiles/gettau.md keeps them."""
import numpy as np
import pytest

from tests import gettau_util as U

CANARY = -7.0
IR_BANDS = (1, 3, 4, 10)
TAUCRIT = 0.30
K_LOG10 = U.K_LOG10


@pytest.fixture(scope="module")
def gtref(tmp_path_factory):
    return U.build_ref(tmp_path_factory.mktemp("gettau_gpu"))


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def _shapes(kind, nlevs, ncol):
    if kind == "ir":
        return {"taudiag": (4, nlevs, ncol), "tcldlyr": (nlevs + 1, ncol), "enn": (nlevs + 1, ncol)}
    s = {"taubeam": (4, nlevs, ncol), "taudiff": (4, nlevs, ncol), "asycl": (nlevs, ncol)}
    if kind == "nir":
        s["ssacl"] = (nlevs, ncol)
    return s


def dev_call(ctx, kind, a, ib=0, ict=0, icb=0, want=None, drop=()):
    """the `_dev` entry point on device copies of `a`; every output is allocated and canary-filled, those in `want` (default all) are passed"""
    import torch
    dt = ctx.dtype
    nlevs, ncol = a["dp"].shape
    t = {k: torch.from_numpy(np.ascontiguousarray(a[k], dtype=dt)).cuda() for k in ("cosz", "dp", "fcld", "reff", "hyd")}
    shapes = _shapes(kind, nlevs, ncol)
    o = {k: torch.full(s, CANARY, dtype=t["dp"].dtype, device="cuda") for k, s in shapes.items()}
    ptr = {"cosz": t["cosz"].data_ptr(), "dp": t["dp"].data_ptr(), "fcld": t["fcld"].data_ptr(), "reff": t["reff"].data_ptr(),
           "hydromets": t["hyd"].data_ptr()}
    for k in drop:
        del ptr[k]
    ptr.update({k: o[k].data_ptr() for k in (shapes if want is None else want)})
    st = _stream()
    try:
        if kind == "vis":
            ctx.getvistau_dev(st, ncol, nlevs, ptr, ict, icb)
        elif kind == "nir":
            ctx.getnirtau_dev(st, ib, ncol, nlevs, ptr, ict, icb)
        else:
            ctx.getirtau_dev(st, ib, ncol, nlevs, ptr)
        ctx.check(st)
    finally:
        torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in o.items()}


def host_call(ctx, kind, a, ib=0, ict=0, icb=0, **kw):
    nlevs, ncol = a["dp"].shape
    if kind == "vis":
        return ctx.getvistau(ncol, nlevs, a["cosz"], a["dp"], a["fcld"], a["reff"], a["hyd"], ict, icb, **kw)
    if kind == "nir":
        return ctx.getnirtau(ib, ncol, nlevs, a["cosz"], a["dp"], a["fcld"], a["reff"], a["hyd"], ict, icb, **kw)
    return ctx.getirtau(ib, ncol, nlevs, a["dp"], a["fcld"], a["reff"], a["hyd"], **kw)


MEASURED = {}


def _note(key, value):
    MEASURED[key] = max(MEASURED.get(key, 0.0), float(value))


def _rel(got, ref, atol=0.0):
    g, r = got.astype(np.float64), ref.astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        e = np.where(g == r, 0.0, np.abs(g - r) / np.maximum(np.abs(r), 1e-300))
    return np.where(np.abs(g - r) <= atol, 0.0, e)


def check_sw(got, ref, unsc, rk, scaled, tag):
    """getvistau / getnirtau outputs against the restatement (module docstring)"""
    dt = np.float32 if rk == 4 else np.float64
    eps = float(np.finfo(dt).eps)
    rtol, atol = (2e-6, 0.0) if rk == 4 else (1e-12, 1e-12)
    for k in got:
        # an undefined radius is 1e21 microns here (synth_batch): in fp32 the polynomials of asycl / ssacl overflow for it, in the reference as
        # in the kernel - the same cells must be Inf / NaN on both sides, the others are compared
        fin, inf = np.isfinite(ref[k]), np.isinf(ref[k])
        assert (np.isnan(got[k]) == np.isnan(ref[k])).all() and (got[k][inf] == ref[k][inf]).all(), (tag, k)
        assert fin.mean() > 0.8 and (fin.all() or (rk == 4 and k in ("asycl", "ssacl"))), (tag, k)
        g, r = np.where(fin, got[k], 0), np.where(fin, ref[k], 0)
        if scaled and k in ("taubeam", "taudiff"):
            d = np.abs(g.astype(np.float64) - r.astype(np.float64))
            u = U.ulp(g, r)
            bound = K_LOG10 * eps * unsc + 2 * np.spacing(np.abs(r)).astype(np.float64)
            _note((rk, k, "scaled: eps of the unscaled thickness"), (d / np.maximum(eps * unsc, 1e-300)).max() if d.any() else 0.0)
            _note((rk, k, "scaled: cells differing"), (u > 0).sum())
            _note((rk, k, "scaled: cells differing by more than 2 ulp"), (u > 2).sum())
            assert (d <= bound).all(), (tag, k, int((d > bound).sum()), float(u.max()))
            assert ((r == 0) == (g == 0)).all(), (tag, k)      # a thin or uncovered layer: exactly zero on both sides
        else:
            e = _rel(g, r, atol)
            _note((rk, k, "rel"), e.max())
            assert (e <= rtol).all(), (tag, k, float(e.max()))


def check_ir(got, ref, rk, tag):
    for k in got:
        assert np.isfinite(got[k]).all(), (tag, k)
        if rk == 8:
            e = _rel(got[k], ref[k], 1e-12)
            _note((rk, k, "rel"), e.max())
            assert (e <= 1e-12).all(), (tag, k, float(e.max()))
        elif k == "taudiag":
            e = _rel(got[k], ref[k])
            _note((rk, k, "rel"), e.max())
            assert (e <= 2e-4).all(), (tag, k, float(e.max()))
        else:
            d = np.abs(got[k].astype(np.float64) - ref[k].astype(np.float64))
            _note((rk, k, "abs"), d.max())
            assert (d <= 7.4e-5).all(), (tag, k, float(d.max()))
    if "tcldlyr" in got:
        assert (got["tcldlyr"][0] == 1).all() and (got["enn"][0] == 0).all()


def _sweep(ctx, gtref, rk, a, modes, tag, a_ir=None):
    """getvistau and getnirtau 1-3 in every mode on the batch `a`, getirtau on `a_ir` (default `a`)"""
    for ict, icb in modes:
        for kind, ib in (("vis", 0), ("nir", 1), ("nir", 2), ("nir", 3)):
            got = dev_call(ctx, kind, a, ib, ict, icb)
            ref = gtref.swtau(ib, a, ict, icb, rk)
            check_sw(got, ref, U.unscaled(gtref, ib, a, rk), rk, ict != 0, f"{tag} {kind}{ib} ict={ict} icb={icb}")
    a_ir = a if a_ir is None else a_ir
    for ib in IR_BANDS:
        check_ir(dev_call(ctx, "ir", a_ir, ib), gtref.irtau(ib, a_ir, rk), rk, f"{tag} ir{ib}")


def _report(capsys, what):
    with capsys.disabled():
        print(f"\n{what}: measured maxima against the restatement")
        for key in sorted(MEASURED, key=str):
            print(f"  r{key[0]} {key[1]:8s} {key[2]}: {MEASURED[key]:.4g}")


@pytest.mark.gpu
@pytest.mark.parametrize("nlevs", [1, 4, 33, 72])
@pytest.mark.parametrize("ncol", [70, 300])
@pytest.mark.parametrize("rk", [4, 8])
def test_kernels_match_restatement(gpu_ctx, gtref, rk, ncol, nlevs, capsys):
    """ncol ragged against 64 and 256; nlevs 1 (one layer run, one layer), 4, 33 (a ragged last run of GT_LC = 8 and of the load pairs), 72;
    modes: in-cloud, the synthetic LCLDMH / LCLDLM, (1, 1) and (nlevs + 1, nlevs + 1) with two empty super-layers each"""
    a, ict, icb = U.synth_batch(ncol, nlevs)
    modes = [(0, 0), (ict, icb), (1, 1), (nlevs + 1, nlevs + 1)]
    if nlevs >= 7:
        modes.append((4, 7))
    _sweep(gpu_ctx[rk], gtref, rk, a, modes, f"r{rk} {ncol}x{nlevs}", a_ir=U.synth_batch(ncol, nlevs, lw=True)[0])
    if (ncol, nlevs) == (300, 72):
        ref = gtref.swtau(0, a, ict, icb, rk)
        assert (ref["asycl"] != 1).sum() > 500 and (ref["taudiff"].sum(axis=0) > 0).sum() > 500      # the batch has cloud
        _report(capsys, f"r{rk} synthetic batches")


@pytest.mark.gpu
@pytest.mark.parametrize("rk", [4, 8])
def test_hand_built_columns(gpu_ctx, gtref, rk, capsys):
    _sweep(gpu_ctx[rk], gtref, rk, U.hand_columns(gtref), U.HAND_MODES, f"r{rk} hand-built")
    _report(capsys, f"r{rk} + hand-built columns")


@pytest.mark.gpu
@pytest.mark.parametrize("rk", [4, 8])
def test_null_outputs_untouched_and_the_rest_unchanged(gpu_ctx, rk):
    ctx = gpu_ctx[rk]
    a, ict, icb = U.synth_batch(300, 33, start=9400)
    a_ir = U.synth_batch(300, 33, start=9400, lw=True)[0]
    for kind, ib, mode in (("vis", 0, (ict, icb)), ("nir", 2, (ict, icb)), ("nir", 3, (0, 0)), ("ir", 4, (0, 0))):
        a = a_ir if kind == "ir" else a
        full = dev_call(ctx, kind, a, ib, *mode)
        names = list(full)
        for sel in [[k] for k in names] + [names[:2], names[1:]]:
            part = dev_call(ctx, kind, a, ib, *mode, want=sel)
            for k in names:
                if k in sel:
                    np.testing.assert_array_equal(part[k], full[k], err_msg=f"{kind} {sel} {k}")
                else:
                    assert (part[k] == CANARY).all(), (kind, sel, k)
    # cosz enters only the beam scaling of the overlap mode: NULL elsewhere
    full = dev_call(ctx, "vis", a, 0, ict, icb)
    nocz = dev_call(ctx, "vis", a, 0, ict, icb, want=["taudiff", "asycl"], drop=("cosz",))
    np.testing.assert_array_equal(nocz["taudiff"], full["taudiff"])
    free = dev_call(ctx, "nir", a, 1, 0, 0, drop=("cosz",))
    np.testing.assert_array_equal(free["taubeam"], dev_call(ctx, "nir", a, 1, 0, 0)["taubeam"])


@pytest.mark.gpu
@pytest.mark.parametrize("rk", [4, 8])
def test_host_variant_chunks_and_shards_are_bitwise_the_dev_result(gpu_ctx, rk):
    from geosradiation_gridcomp_amd.api import Context
    ctx = gpu_ctx[rk]
    a, ict, icb = U.synth_batch(150, 33, start=9500)
    calls = [("vis", 0, (ict, icb)), ("vis", 0, (0, 0)), ("nir", 2, (ict, icb)), ("ir", 3, (0, 0))]
    a_ir = U.synth_batch(150, 33, start=9500, lw=True)[0]
    batch = {"vis": a, "nir": a, "ir": a_ir}
    dev = [dev_call(ctx, kind, batch[kind], ib, *mode) for kind, ib, mode in calls]
    for (kind, ib, mode), d in zip(calls, dev):
        h = host_call(ctx, kind, batch[kind], ib, *mode)
        assert set(h) == set(d)
        for k in d:
            np.testing.assert_array_equal(h[k], d[k], err_msg=f"host {kind} {k}")
    # a subset of the outputs: the others are not staged at all
    h = host_call(ctx, "nir", a, 2, ict, icb, want=("taudiff", "ssacl"))
    assert set(h) == {"taudiff", "ssacl"} and np.array_equal(h["taudiff"], dev[2]["taudiff"]) and np.array_equal(h["ssacl"], dev[2]["ssacl"])
    ctx.set_chunk(64)                       # 150 columns: chunks of 64, 64, 22
    try:
        for (kind, ib, mode), d in zip(calls, dev):
            h = host_call(ctx, kind, batch[kind], ib, *mode)
            for k in d:
                np.testing.assert_array_equal(h[k], d[k], err_msg=f"chunked {kind} {k}")
    finally:
        ctx.set_chunk(131072)
    multi = Context(rk, devices=[0, 0])     # two shards of 75 columns on the one GPU
    try:
        for (kind, ib, mode), d in zip(calls, dev):
            h = host_call(multi, kind, batch[kind], ib, *mode)
            for k in d:
                np.testing.assert_array_equal(h[k], d[k], err_msg=f"sharded {kind} {k}")
    finally:
        multi.close()


@pytest.mark.gpu
@pytest.mark.parametrize("rk", [4, 8])
def test_error_returns_write_nothing(gpu_ctx, rk):
    from geosradiation_gridcomp_amd.api import Context, GeosradError
    ctx = gpu_ctx[rk]
    a, ict, icb = U.synth_batch(70, 4, start=9600)
    bad = [("nir", 0, (ict, icb), {}), ("nir", 4, (ict, icb), {}), ("ir", 0, (0, 0), {}), ("ir", 11, (0, 0), {}),      # ib out of range
           ("vis", 0, (3, 2), {}), ("nir", 1, (3, 2), {}), ("vis", 0, (1, 6), {}), ("vis", 0, (-1, 2), {}),              # ict > icb, icb > nlevs + 1
           ("vis", 0, (ict, icb), {"want": []}), ("nir", 1, (0, 0), {"want": []}), ("ir", 3, (0, 0), {"want": []}),       # all outputs NULL
           ("vis", 0, (ict, icb), {"drop": ("cosz",)}), ("ir", 3, (0, 0), {"drop": ("reff",)})]
    for kind, ib, mode, kw in bad:
        with pytest.raises(GeosradError) as e:
            dev_call(ctx, kind, a, ib, *mode, **kw)
        assert e.value.rc == 1, (kind, ib, mode, kw)
    import torch
    tdt = torch.float32 if rk == 4 else torch.float64
    z = torch.zeros(64, dtype=tdt, device="cuda")
    sent = torch.full((64,), CANARY, dtype=tdt, device="cuda")
    ptr = {k: z.data_ptr() for k in ("cosz", "dp", "fcld", "reff", "hydromets")}
    ptr.update(asycl=sent.data_ptr(), enn=sent.data_ptr())
    for ncol, nlevs in ((4, 0), (0, 4), (-3, 4)):      # nlevs = 0, ncol <= 0
        with pytest.raises(GeosradError):
            ctx.getvistau_dev(_stream(), ncol, nlevs, ptr, 0, 0)
        with pytest.raises(GeosradError):
            ctx.getirtau_dev(_stream(), 3, ncol, nlevs, ptr)
    with pytest.raises(GeosradError):
        ctx.getvistau(4, 0, np.zeros(4), np.zeros((0, 4)), np.zeros((0, 4)), np.zeros((4, 0, 4)), np.zeros((4, 0, 4)), 0, 0)
    with pytest.raises(TypeError):
        ctx.getirtau(3, 4, 1, np.zeros((1, 4)), np.zeros((1, 4)), np.zeros((4, 1, 4)), np.zeros((4, 1, 4)), want=("taubeam",))
    bare = Context(rk, tables=False)
    try:
        with pytest.raises(GeosradError, match="tables not set"):
            bare.getvistau_dev(_stream(), 4, 1, ptr, 0, 0)
        with pytest.raises(GeosradError, match="tables not set"):
            bare.getirtau_dev(_stream(), 3, 4, 1, ptr)
    finally:
        bare.close()
    torch.cuda.synchronize()
    assert (sent == CANARY).all().item()
    # legal edges: empty super-layers
    for mode in ((1, 1), (5, 5), (1, 5), (2, 2)):
        dev_call(ctx, "vis", a, 0, *mode)


# ---- device against device -------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("rk", [4, 8])
def test_species_sum_is_irrads_taudiag(gpu_ctx, rk, capsys):
    """the sum over species of getirtau's taudiag(ib) against TAUDIAG(:,:,ib) of irrad on the same columns"""
    from geosradiation_gridcomp_amd import synth
    ctx = gpu_ctx[rk]
    dt = ctx.dtype
    inp = synth.make_columns(300, 33, start=9700, cloudy_frac=0.7, aerosol=False)
    ch = synth.chou_lw_inputs(inp)
    td = ctx.irrad_columns(ch, trace=True)["taudiag"]                      # (10, np, m)
    ple = np.ascontiguousarray(ch["ple"], dtype=dt)
    a = {"dp": ple[1:] - ple[:-1], "fcld": ch["fcld"], "reff": ch["reff"], "hyd": ch["cwc"], "cosz": np.zeros(300)}      # irrad.F90:645: dp in Pa
    worst = 0.0
    for ib in IR_BANDS:
        t = host_call(ctx, "ir", a, ib, want=("taudiag",))["taudiag"]
        e = _rel(((t[0] + t[1]) + t[2]) + t[3], td[ib - 1], 1e-12 if rk == 8 else 0.0)
        worst = max(worst, float(e.max()))
        assert (e <= (2e-4 if rk == 4 else 1e-12)).all(), (ib, float(e.max()))
    assert (td[2] > 0).sum() > 100
    with capsys.disabled():
        print(f"\nr{rk} sum of species against irrad's TAUDIAG: largest relative difference {worst:.3g}")


def lw_fields(ncol, lm, start=9800):
    """GEOS fields of LW_Driver (synth.geos_chou_lw_fields: MAPL_UNDEF radii in every 7th cell) with column 5 free of cloud; float64"""
    from geosradiation_gridcomp_amd import synth
    inp = synth.make_columns(ncol, lm, start=start, cloudy_frac=0.7, aerosol=True)
    f = synth.geos_chou_lw_fields(inp, aerosol=False)
    for k in ("FCLD", "QI", "QL", "QR", "QS"):
        f[k][:, 5] = 0.0
    return f


def near_taucrit(tauir, dt, taucrit=TAUCRIT):
    """columns with a layer whose TAUIR lies within 2 ulp of TAUCRIT / 2.13 (the division in the real kind)"""
    crit = dt(taucrit) / dt(2.13)
    return (np.abs(tauir.astype(np.float64) - np.float64(crit)) <= 2 * float(np.spacing(crit))).any(axis=0)


@pytest.mark.gpu
@pytest.mark.parametrize("rk", [4, 8])
def test_lw_cloud_diag_equals_the_chou_driver(gpu_ctx, gtref, rk, capsys):
    """TAUIR / CLDTMP / CLDPRS of geosrad_lw_cloud_diag_dev against those of geosrad_lw_driver_chou_dev on the same GEOS fields"""
    import torch
    from geosradiation_gridcomp_amd import gridcomp as G
    ctx = gpu_ctx[rk]
    dt = ctx.dtype
    ncol, lm = 300, 72
    f = lw_fields(ncol, lm)
    fields = {k: np.ascontiguousarray(f[k], dtype=dt) for k in G.LWK_IN if k in f}
    undef = float(dt(G.MAPL["UNDEF"]))
    consts = G.lwk_consts(co2=f["CO2"], UNDEF=undef, TAUCRIT=TAUCRIT)
    tin = {k: torch.from_numpy(v.copy()).cuda() for k, v in fields.items()}
    shape = lambda k: (lm + 1, ncol) if k in G.LWK_OUT_REQUIRED[:9] else (lm, ncol) if k == "TAUIR" else (ncol,)
    names = G.LWK_OUT_REQUIRED + ["TAUIR", "CLDTMP", "CLDPRS"]
    tout = {k: torch.full(shape(k), CANARY, dtype=tin["T"].dtype, device="cuda") for k in names}
    ptr = {k: v.data_ptr() for k, v in tin.items()}
    ptr.update({k: v.data_ptr() for k, v in tout.items()})
    st = _stream()
    ctx.lw_driver_chou_dev(st, ncol, lm, ptr, consts, True, f["LCLDMH"], f["LCLDLM"])
    ctx.check(st)
    want = {k: tout[k].cpu().numpy() for k in ("TAUIR", "CLDTMP", "CLDPRS")}
    mine = {k: torch.full(shape(k), CANARY, dtype=tin["T"].dtype, device="cuda") for k in ("TAUIR", "CLDTMP", "CLDPRS")}
    p2 = {k: tin[k].data_ptr() for k in ("PLE", "T", "FCLD", "QI", "QL", "QR", "QS", "RI", "RL", "RR", "RS")}
    p2.update({k: v.data_ptr() for k, v in mine.items()})
    ctx.lw_cloud_diag_dev(st, ncol, lm, p2, taucrit=TAUCRIT, undef=undef)
    ctx.check(st)
    torch.cuda.synchronize()
    got = {k: v.cpu().numpy() for k, v in mine.items()}
    u = U.ulp(got["TAUIR"], want["TAUIR"])
    assert u.max() <= 2, float(u.max())
    near = near_taucrit(want["TAUIR"], dt) | near_taucrit(got["TAUIR"], dt)
    assert near.mean() <= 0.01
    for k in ("CLDTMP", "CLDPRS"):
        assert (got[k][~near] == want[k][~near]).all(), k
    assert got["CLDTMP"][5] == dt(undef) and got["CLDPRS"][5] == dt(undef) and (got["TAUIR"][:, 5] == 0).all()
    assert (got["CLDTMP"] != dt(undef)).mean() > 0.3 and (fields["RI"] == dt(undef)).sum() > 100
    # each export alone; FCLD and RR do not enter
    for sel in (["TAUIR"], ["CLDTMP"], ["CLDPRS"]):
        one = {k: torch.full(shape(k), CANARY, dtype=tin["T"].dtype, device="cuda") for k in mine}
        p3 = {k: v for k, v in p2.items() if k not in mine and k not in ("FCLD", "RR")}
        p3.update({k: one[k].data_ptr() for k in sel})
        ctx.lw_cloud_diag_dev(st, ncol, lm, p3, taucrit=TAUCRIT, undef=undef)
        torch.cuda.synchronize()
        for k in mine:
            assert torch.equal(one[k], mine[k]) if k in sel else bool((one[k] == CANARY).all()), (sel, k)
    # the restatement on the same fields: fp64 to 1e-12, fp32 to the bound of taudiag
    r = gtref.lw_cloud_diag(fields, rk, taucrit=TAUCRIT, undef=undef)
    e = _rel(got["TAUIR"], r["TAUIR"], 1e-12 if rk == 8 else 0.0)
    assert (e <= (2e-4 if rk == 4 else 1e-12)).all(), float(e.max())
    with capsys.disabled():
        print(f"\nr{rk} lw_cloud_diag against lw_driver_chou: TAUIR cells differing {int((u > 0).sum())} of {u.size}, worst {u.max():g} ulp; "
              f"columns next to TAUCRIT / 2.13: {int(near.sum())}; cloud tops that differ: {int((got['CLDTMP'] != want['CLDTMP']).sum())}; "
              f"TAUIR against the restatement: {e.max():.3g}")
    from geosradiation_gridcomp_amd.api import GeosradError
    with pytest.raises(GeosradError):
        ctx.lw_cloud_diag_dev(st, ncol, lm, {k: v for k, v in p2.items() if k not in mine}, taucrit=TAUCRIT)      # all outputs NULL
    with pytest.raises(GeosradError):
        ctx.lw_cloud_diag_dev(st, ncol, 0, p2, taucrit=TAUCRIT)
    with pytest.raises(GeosradError):
        ctx.lw_cloud_diag_dev(st, ncol, lm, {k: v for k, v in p2.items() if k != "QL"}, taucrit=TAUCRIT)
