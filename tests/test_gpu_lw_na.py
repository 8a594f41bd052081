"""GPU tests of the aerosol-free RRTMG_LW fluxes from one shared call: geosrad_rrtmg_lw_na[_dev] (the six flux arrays of the same
columns with tauaer taken away) and geosrad_lw_driver_rrtmg_na_dev (the INTERNALs FLXAU / FLXAD / FLAU / FLAD / FLXA / FLA and the real
DFDTSNA / DFDTSCNA, which the reference's RRTMG branch leaves undefined, GEOS_IrradGridComp.F90:3552-3556).  The reference has no value
for them, so the yardstick is the library's own existing entry point called with the aerosols taken away: every comparison is bitwise."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

from geosradiation_gridcomp_amd import gridcomp as G
from geosradiation_gridcomp_amd import synth
from tests.conftest import FLUX, ROOT

pytestmark = pytest.mark.gpu
NA = tuple(k + "_na" for k in FLUX)
RAT = ("uflx_rat", "dflx_rat", "duflx_dTs_rat")
NAMES = ["play", "plev", "tlay", "tlev", "tsfc", "emis", "zm", "alat"] + list(G.RAT_VMR.values()) + \
        ["o2vmr", "ccl4vmr", "cldf", "ciwp", "clwp", "rei", "rel"]
SLOT_SWEEP, SLOT_REDUCE = 4, 5          # geosrad_profile_read: the band sweeps and the band reduction of RRTMG_LW


@functools.lru_cache(maxsize=None)
def columns(ncol, nlay, cloudy_frac=0.6):
    """cloudy and clear columns mixed, aerosols on (shared between the tests, never modified)"""
    return synth.make_columns(ncol, nlay, start=1313, cloudy_frac=cloudy_frac, aerosol=True)


def launches(ctx, slot):
    import ctypes
    ms = ctypes.c_double(); n = ctypes.c_long()
    ctx._chk(ctx.L.geosrad_profile_read(ctx.h, ctypes.c_int(slot), ctypes.byref(ms), ctypes.byref(n)))
    return n.value


def lw_dev(ctx, inp, entry, aer="given", gases=(), chunk=131072, dudTs=True, counts=None):
    """geosrad_rrtmg_lw_na_dev (entry "na") or geosrad_rrtmg_lw_rats_dev ("rats") on device copies of `inp`; tauaer as `inp` has it
    ("given"), an array of exact zeros ("zero") or NULL (None).  Every output as numpy; untouched outputs keep the poison -7.
    counts: a dict that receives the number of band sweeps and reductions the call enqueued."""
    import torch
    nlay, ncol = inp["play"].shape
    t = {k: torch.from_numpy(np.ascontiguousarray(inp[k], dtype=ctx.dtype)).cuda() for k in NAMES}
    if aer is not None:
        ta = np.ascontiguousarray(inp["tauaer"], dtype=ctx.dtype)
        t["tauaer"] = torch.from_numpy(ta if aer == "given" else np.zeros_like(ta)).cuda()
    tdt = t["play"].dtype
    outs = FLUX + (NA if entry == "na" else ())
    for k in outs:
        t[k] = torch.full((nlay + 1, ncol), -7.0, dtype=tdt, device="cuda")
    for k in RAT:
        t[k] = torch.full((max(len(gases), 1), nlay + 1, ncol), -7.0, dtype=tdt, device="cuda")
    t["clearCounts"] = torch.zeros((4, ncol), dtype=torch.int32, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    fn = ctx.rrtmg_lw_na_dev if entry == "na" else ctx.rrtmg_lw_rats_dev
    ctx.set_chunk(chunk)
    try:
        if counts is not None:
            ctx.profile(True)
        fn(st, ncol, nlay, dudTs, {k: v.data_ptr() for k, v in t.items()}, 3, 1, int(inp["dyofyr"]), int(inp["cloudLM"]),
           int(inp["cloudMH"]), list(gases))
        ctx.check(st)
        if counts is not None:
            counts["sweeps"] = launches(ctx, SLOT_SWEEP); counts["reductions"] = launches(ctx, SLOT_REDUCE)
    finally:
        if counts is not None:
            ctx.profile(False)
        ctx.set_chunk(131072)
    return {k: t[k].cpu().numpy() for k in outs + RAT + ("clearCounts",)}


_cache = {}


def shared(ctx, rk, key, **kw):
    """one call per (precision, arguments) for the tests that compare against it"""
    if (rk, key) not in _cache:
        _cache[(rk, key)] = lw_dev(ctx, **kw)
    return _cache[(rk, key)]


def check_na_equals_call_without_aerosols(ctx, rk, inp, tag):
    a = shared(ctx, rk, ("na", tag), inp=inp, entry="na")
    b = lw_dev(ctx, inp, "rats", aer=None, gases=["CO2"])          # nrats = 1: the same band-partials path
    c = lw_dev(ctx, inp, "rats", aer="given", gases=["CO2"])
    for k in FLUX:
        assert np.array_equal(a[k + "_na"], b[k]), k + "_na"
        assert np.array_equal(a[k], c[k]), k
    assert np.array_equal(a["clearCounts"], c["clearCounts"])
    assert (a["clearCounts"][0] > 0).any() and (a["clearCounts"][0] < 140).any()      # clear and cloudy columns
    assert np.isfinite(a["uflx_na"]).all() and not np.array_equal(a["dflx_na"], a["dflx"])      # the aerosols do absorb
    return a


@pytest.mark.parametrize("rk", [8, 4])
def test_aerosol_free_fluxes_equal_a_call_without_aerosols(gpu_ctx, rk):
    """300 columns (two 256-thread blocks, the second ragged) x 33 layers: the six _na arrays are the bits of uflx .. duflxc_dTs of
    geosrad_rrtmg_lw_rats_dev with tauaer = NULL, the with-aerosol outputs and clearCounts those of that entry point with tauaer given"""
    check_na_equals_call_without_aerosols(gpu_ctx[rk], rk, columns(300, 33), "300x33")


def test_aerosol_free_fluxes_through_the_wide_cloud_free_blocks(gpu_ctx):
    """1100 columns x 72 layers, mostly cloud-free, fp32: the 768-thread cloud-free blocks run"""
    inp = columns(1100, 72, cloudy_frac=0.05)
    a = check_na_equals_call_without_aerosols(gpu_ctx[4], 4, inp, "1100x72")
    assert (a["clearCounts"][0] == 140).mean() > 0.8


@pytest.mark.parametrize("rk", [8, 4])
def test_zero_aerosols_are_no_aerosols(gpu_ctx, rk):
    """tauaer an array of exact zeros: every _na array equals its with-aerosol twin (a reduction that read the wrong partial buffer for
    some band would differ).  tauaer = NULL: the same, and the band sweeps ran once per chunk, the reduction twice"""
    ctx = gpu_ctx[rk]
    inp = columns(300, 33)
    z = lw_dev(ctx, inp, "na", aer="zero")
    for k in FLUX:
        assert np.array_equal(z[k + "_na"], z[k]), k
    n = {}
    o = lw_dev(ctx, inp, "na", aer=None, counts=n)
    for k in FLUX:
        assert np.array_equal(o[k + "_na"], o[k]), k
        assert np.array_equal(o[k], z[k]), k          # exact zeros add nothing
    assert n == {"sweeps": 1, "reductions": 2}, n
    n = {}
    lw_dev(ctx, inp, "na", aer="given", counts=n)
    assert n == {"sweeps": 2, "reductions": 2}, n


@pytest.mark.parametrize("rk", [8, 4])
def test_with_rats_the_second_partials_are_reused_in_order(gpu_ctx, rk):
    """nrats = 2 (CO2, H2O) together with the _na arrays: the RATS outputs are those of geosrad_rrtmg_lw_rats_dev, the _na outputs those
    of the call without RATS - the aerosol-free pass and the RATS passes share one second set of band partials, one after the other"""
    ctx = gpu_ctx[rk]
    inp = columns(300, 33)
    gases = ["CO2", "H2O"]
    a = lw_dev(ctx, inp, "na", gases=gases)
    r = lw_dev(ctx, inp, "rats", gases=gases)
    base = shared(ctx, rk, ("na", "300x33"), inp=inp, entry="na")
    for k in FLUX + RAT + ("clearCounts",):
        assert np.array_equal(a[k], r[k]), k
    for k in NA:
        assert np.array_equal(a[k], base[k]), k
    for g in range(2):
        assert not np.array_equal(a["uflx_rat"][g], a["uflx"]) and (a["uflx_rat"][g] != -7.0).all()


@pytest.mark.parametrize("rk", [8, 4])
def test_chunking_is_invisible(gpu_ctx, rk):
    """600 columns with geosrad_set_chunk(256): three chunks, the last ragged, against one chunk"""
    ctx = gpu_ctx[rk]
    inp = columns(600, 33)
    n = {}
    whole = lw_dev(ctx, inp, "na", gases=["CO2"])
    chunked = lw_dev(ctx, inp, "na", gases=["CO2"], chunk=256, counts=n)
    assert n["sweeps"] == 3 * 3, n          # main, aerosol-free and one gas, per chunk
    for k in FLUX + NA + RAT + ("clearCounts",):
        assert np.array_equal(chunked[k], whole[k]), k


def run_split_path_child():
    """test 1 under the kernel path GEOSRAD_LW_PATH selects (read by geosrad_create): run in a child process"""
    from geosradiation_gridcomp_amd.api import Context
    for rk in (8, 4):
        ctx = Context(rk)
        try:
            check_na_equals_call_without_aerosols(ctx, rk, columns(300, 33), "child")
        finally:
            ctx.close()


def test_the_split_path():
    """the same bitwise statement within the two-kernel band sweeps (GEOSRAD_LW_PATH=split), in a fresh child process"""
    env = dict(os.environ, GEOSRAD_LW_PATH="split")
    flags = ["-s"] if sys.flags.no_user_site else []
    r = subprocess.run([sys.executable, *flags, "-c", "import tests.test_gpu_lw_na as t; t.run_split_path_child(); print('split ok')"],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "split ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


@pytest.mark.parametrize("rk", [8, 4])
def test_host_pointers_through_the_chunked_pipeline(rk):
    """geosrad_rrtmg_lw_na at 300 columns with GEOSRAD_HOST_CHUNK = 128 (three host chunks, the last ragged): the _dev results; a
    two-shard context gives them too"""
    from geosradiation_gridcomp_amd.api import Context
    inp = columns(300, 33)
    old = os.environ.get("GEOSRAD_HOST_CHUNK")
    os.environ["GEOSRAD_HOST_CHUNK"] = "128"          # read by geosrad_create
    try:
        ctx = Context(rk)
    finally:
        if old is None:
            del os.environ["GEOSRAD_HOST_CHUNK"]
        else:
            os.environ["GEOSRAD_HOST_CHUNK"] = old
    try:
        h = ctx.rrtmg_lw_na_columns(inp)
        d = lw_dev(ctx, inp, "na")
        plain = ctx.rrtmg_lw_columns(inp)
        nd = ctx.rrtmg_lw_na_columns(inp, dudTs=False)          # the derivative arrays are ignored
    finally:
        ctx.close()
    two = Context(rk, devices=[0, 0])          # geosrad_create_multi: two shards of 150 columns, the _na rows sharded like uflx
    try:
        m = two.rrtmg_lw_na_columns(inp)
    finally:
        two.close()
    for k in FLUX + NA + ("clearCounts",):
        assert np.array_equal(m[k], h[k]), k
    for k in FLUX + NA + ("clearCounts",):
        assert np.array_equal(h[k], d[k]), k
    for k in FLUX:          # the default path: the plain entry point's bits too
        assert np.array_equal(h[k], plain[k]), k
    for k in ("uflx_na", "dflx_na", "uflxc_na", "dflxc_na"):
        assert np.array_equal(nd[k], h[k]), k
    assert not nd["duflx_dTs_na"].any() and not nd["duflx_dTs"].any()


def test_argument_validation_launches_nothing(gpu_ctx):
    """a required _na array NULL, dudTs with a derivative array NULL, nrats > 8: GEOSRAD_EINVAL and no kernel"""
    import torch
    from geosradiation_gridcomp_amd.api import GeosradError
    ctx = gpu_ctx[4]
    inp = columns(300, 33)
    nlay, ncol = inp["play"].shape
    t = {k: torch.from_numpy(np.ascontiguousarray(inp[k], dtype=np.float32)).cuda() for k in NAMES + ["tauaer"]}
    for k in FLUX + NA:
        t[k] = torch.full((nlay + 1, ncol), -7.0, device="cuda")
    for k in RAT:
        t[k] = torch.full((9, nlay + 1, ncol), -7.0, device="cuda")
    t["clearCounts"] = torch.zeros((4, ncol), dtype=torch.int32, device="cuda")
    ptr = {k: v.data_ptr() for k, v in t.items()}
    st = torch.cuda.current_stream().cuda_stream
    tail = (3, 1, int(inp["dyofyr"]), int(inp["cloudLM"]), int(inp["cloudMH"]))
    ctx.profile(True)
    try:
        for drop, dud in (("uflx_na", True), ("dflx_na", False), ("uflxc_na", True), ("dflxc_na", False), ("duflx_dTs_na", True),
                          ("duflxc_dTs_na", True)):
            bad = dict(ptr); bad[drop] = 0
            with pytest.raises(GeosradError, match="must not be null") as e:
                ctx.rrtmg_lw_na_dev(st, ncol, nlay, dud, bad, *tail)
            assert e.value.rc == 1          # GEOSRAD_EINVAL
        with pytest.raises(GeosradError, match="bad RATS") as e:
            ctx.rrtmg_lw_na_dev(st, ncol, nlay, True, ptr, *tail, list(range(8)) + [0])
        assert e.value.rc == 1
        assert [launches(ctx, k) for k in range(6)] == [0] * 6
        # without dudTs the derivative arrays are ignored
        ok = dict(ptr); ok["duflx_dTs_na"] = 0; ok["duflxc_dTs_na"] = 0
        ctx.rrtmg_lw_na_dev(st, ncol, nlay, False, ok, *tail)
        ctx.check(st)
    finally:
        ctx.profile(False)
    for k in FLUX + NA:
        assert ((t[k] == -7.0).all().item()) == (k.startswith("du")), k


# ---- GridComp level -----------------------------------------------------------------------------------------------------------

def _dev(arrs, dt):
    import torch
    t = {k: torch.from_numpy(np.ascontiguousarray(v, dtype=dt)).cuda() for k, v in arrs.items() if isinstance(v, np.ndarray)}
    return t, {k: v.data_ptr() for k, v in t.items()}


def _poison(shapes, dt):
    import torch
    tdt = torch.float32 if dt == np.float32 else torch.float64
    t = {k: torch.full(s, -7.0, dtype=tdt, device="cuda") for k, s in shapes.items()}
    return t, {k: v.data_ptr() for k, v in t.items()}


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


@pytest.mark.parametrize("rk", [8, 4])
def test_driver_fills_the_aerosol_free_internals(gpu_ctx, rk):
    from oracle import clib
    ctx = gpu_ctx[rk]; dt = ctx.dtype
    ncol, lm = 300, 33
    inp = columns(ncol, lm)
    f = synth.geos_lw_fields(inp)
    consts = G.lwd_consts()
    doy, llm, lmh = int(inp["dyofyr"]), f["LCLDLM"], f["LCLDMH"]
    tin, pin = _dev(f, dt)
    shapes = {k: ((lm + 1, ncol) if k in G.LWD_OUT_3D else ((ncol, 16) if k in ("OLRB", "DOLRB") else (ncol,))) for k in G.LWD_OUT}
    shapes.update({k: (2, lm + 1, ncol) for k in G.LWD_RAT_OUT[:4]}, SFCEM_RAT=(2, ncol))
    gases = ["CO2", "H2O"]

    def driver(na_names, fields=pin, rats=True):
        """one driver call into fresh poisoned outputs: (out + rat_out, na_out, band sweeps) as numpy"""
        tout, pout = _poison(shapes, dt)
        tna, pna = _poison({k: (lm + 1, ncol) for k in G.LWNA_OUT}, dt)
        ptr = dict(fields); ptr.update(pout)
        ctx.profile(True)
        try:
            if na_names == "rats entry":
                ctx.lw_driver_rrtmg_rats_dev(_stream(), ncol, lm, 16, ptr, consts, 3, 1, doy, llm, lmh, gases)
            else:
                ctx.lw_driver_rrtmg_na_dev(_stream(), ncol, lm, 16, ptr, consts, 3, 1, doy, llm, lmh,
                                           None if na_names is None else {k: pna[k] for k in na_names}, gases if rats else ())
            ctx.check(_stream())
            n = launches(ctx, SLOT_SWEEP)
        finally:
            ctx.profile(False)
        return {k: v.cpu().numpy() for k, v in tout.items()}, {k: v.cpu().numpy() for k, v in tna.items()}, n

    want, _, n_rats = driver("rats entry")
    got, na, n_na = driver(G.LWNA_OUT)
    assert n_rats == 3 and n_na == 4          # main + two gases; the aerosol-free pass adds one sweep
    for k in shapes:
        np.testing.assert_array_equal(got[k], want[k], err_msg=k)          # out and rat_out: the RATS entry point's bits
    # DFDTSNA / DFDTSCNA of `out` keep the reference's meaning: copies
    np.testing.assert_array_equal(got["DFDTSNA"], got["DFDTS"]); np.testing.assert_array_equal(got["DFDTSCNA"], got["DFDTSC"])

    # the solver-level _na arrays from the driver's own prepared inputs, un-flipped in numpy (IRR:3506-3515, :3604-3607)
    rr = clib.lwd_prep(f, consts, 3, 1, {4: "f32", 8: "f64"}[rk])
    inp2 = dict(rr); inp2.update(dyofyr=inp["dyofyr"], cloudLM=inp["cloudLM"], cloudMH=inp["cloudMH"])
    s = lw_dev(ctx, inp2, "na")
    un = lambda a: a[::-1]
    exp = {"FLXAU_INT": -un(s["uflx_na"]), "FLXAD_INT": un(s["dflx_na"]), "FLAU_INT": -un(s["uflxc_na"]), "FLAD_INT": un(s["dflxc_na"]),
           "DFDTSNA": -un(s["duflx_dTs_na"]), "DFDTSCNA": -un(s["duflxc_dTs_na"])}
    exp["FLXA_INT"] = exp["FLXAD_INT"] + exp["FLXAU_INT"]; exp["FLA_INT"] = exp["FLAD_INT"] + exp["FLAU_INT"]
    for k in G.LWNA_OUT:
        np.testing.assert_array_equal(na[k], exp[k], err_msg=k)
    np.testing.assert_array_equal(na["FLXA_INT"], na["FLXAD_INT"] + na["FLXAU_INT"])
    np.testing.assert_array_equal(got["FLXU_INT"], -un(s["uflx"]))
    assert not np.array_equal(na["DFDTSNA"], got["DFDTS"]) and not np.array_equal(na["FLXA_INT"], got["FLX_INT"])

    # a plain-driver call with the aerosol inputs NULL gives the same thing
    noaer = {k: v for k, v in pin.items() if k not in ("TAUA", "SSAA")}
    tout, pout = _poison(shapes, dt)
    ptr = dict(noaer); ptr.update(pout)
    ctx.lw_driver_rrtmg_dev(_stream(), ncol, lm, 0, ptr, consts, 3, 1, doy, llm, lmh)
    ctx.check(_stream())
    for a, b in (("FLXAU_INT", "FLXU_INT"), ("FLXAD_INT", "FLXD_INT"), ("FLAU_INT", "FLCU_INT"), ("FLAD_INT", "FLCD_INT"),
                 ("FLXA_INT", "FLX_INT"), ("FLA_INT", "FLC_INT"), ("DFDTSNA", "DFDTS"), ("DFDTSCNA", "DFDTSC")):
        np.testing.assert_array_equal(na[a], tout[b].cpu().numpy(), err_msg=a)

    # NULL members of na_out are left untouched; with all of them NULL, or na_out NULL, no second sweep runs
    some = ["FLXA_INT", "DFDTSCNA"]
    got2, na2, n2 = driver(some, rats=False)
    assert n2 == 2
    for k in G.LWNA_OUT:
        if k in some:
            np.testing.assert_array_equal(na2[k], na[k], err_msg=k)
        else:
            assert (na2[k] == -7.0).all(), k
    for k in G.LWD_OUT:
        np.testing.assert_array_equal(got2[k], want[k], err_msg=k)
    for none in ([], None):
        got3, na3, n3 = driver(none)
        assert n3 == 3 and all((v == -7.0).all() for v in na3.values())
        for k in shapes:
            np.testing.assert_array_equal(got3[k], want[k], err_msg=k)

    # Update_Flx with the RRTMG semantics off reads the INTERNALs as real fields (IRR:3861-3999)
    u = {"TS_INT": got["TS_INT"], "SFCEM_INT": got["SFCEM_INT"], "FCLD": np.asarray(f["FCLD"], dtype=dt), "TSINST": got["TS_INT"] + dt(1.5)}
    u.update({k: got[k] for k in ("FLX_INT", "FLC_INT", "FLXU_INT", "FLCU_INT", "FLXD_INT", "FLCD_INT", "DFDTS", "DFDTSC")})
    u.update({k: na[k] for k in G.LWNA_OUT})
    exports = ["FLXA", "FLA", "OLRA", "OLA", "LWSA", "LAS", "FLNSNA", "FLNSA", "FLX", "OLR"]
    tu, pu = _dev(u, dt)
    tx, px = _poison({k: ((lm + 1, ncol) if k in G.LWU_OUT_3D else (ncol,)) for k in exports}, dt)
    pu.update(px)
    undef = G.MAPL["UNDEF"]
    ctx.lw_update_flx_dev(_stream(), ncol, lm, False, lmh, llm, undef, pu)
    ctx.check(_stream())
    x = {k: v.cpu().numpy() for k, v in tx.items()}
    delt = u["TSINST"] - u["TS_INT"]
    flxa = na["FLXA_INT"] + na["DFDTSNA"] * delt
    fla = na["FLA_INT"] + na["DFDTSCNA"] * delt
    np.testing.assert_array_equal(x["FLXA"], flxa); np.testing.assert_array_equal(x["FLA"], fla)
    np.testing.assert_array_equal(x["OLRA"], -flxa[0]); np.testing.assert_array_equal(x["OLA"], -fla[0])
    np.testing.assert_array_equal(x["LWSA"], na["FLXA_INT"][lm] + got["SFCEM_INT"])
    np.testing.assert_array_equal(x["LAS"], na["FLA_INT"][lm] + got["SFCEM_INT"])
    np.testing.assert_array_equal(x["FLNSNA"], flxa[lm]); np.testing.assert_array_equal(x["FLNSA"], fla[lm])
    for k in ("FLXA", "FLA", "OLRA", "LWSA"):
        assert (x[k] != dt(undef)).all() and np.isfinite(x[k]).all(), k
    assert (x["OLRA"] > 100).all() and not np.array_equal(x["OLRA"], x["OLR"])

    # the parent's heating rates: RADLWCNA from FLA (GEOS_RadiationGridComp.F90:798-819)
    rt = {"PLE": np.asarray(f["PLE"], dtype=dt), "FLA": x["FLA"]}
    tr, pr = _dev(rt, dt)
    to, po = _poison({"RADLWCNA": (lm, ncol)}, dt)
    pr.update(po)
    ctx.rad_tendencies_dev(_stream(), ncol, lm, G.MAPL["GRAV"], G.MAPL["CP"], pr)
    ctx.check(_stream())
    dmi = dt(G.MAPL["GRAV"]) / (dt(G.MAPL["CP"]) * (rt["PLE"][1:] - rt["PLE"][:-1]))
    np.testing.assert_array_equal(to["RADLWCNA"].cpu().numpy(), (x["FLA"][:-1] - x["FLA"][1:]) * dmi)
