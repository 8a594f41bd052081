"""GPU: the aerosol-free Chou-Suarez shortwave fluxes from one shared call (geosrad_sorad_na / geosrad_sorad_na_dev).  The Solar GridComp
gets FSWNAN ... by running SORADCORE a second time with zero aerosol arrays (GEOS_SolarGridComp.F90:3249-3259, :4541-4551); the yardstick
of every aerosol-free array is therefore this library's existing entry point called with the aerosols taken away, bit for bit
(np.array_equal throughout).  Outputs start poisoned (-7) so that "left untouched" is visible."""
import ctypes
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

IN = ("cosz", "pl", "ta", "wa", "oa", "cwc", "fcld", "reff", "taua", "ssaa", "asya", "rsuvbm", "rsuvdf", "rsirbm", "rsirdf")
PROFILES = ("flx", "flc", "flxu", "flcu")
OUT = PROFILES + ("fdiruv", "fdifuv", "fdirpar", "fdifpar", "fdirir", "fdifir", "flx_sfc_band", "drband", "dfband")      # the 13 regular outputs
NA = ("flx_na", "flc_na", "flxu_na", "flcu_na", "flx_sfc_band_na")
TWIN = dict(zip(NA, ("flx", "flc", "flxu", "flcu", "flx_sfc_band")))
SLOT_PREP, SLOT_PASS = 12, 13           # geosrad_profile_read: sorad's preparation and its spectral passes
POISON = -7.0
EINVAL = 1
NCOL, NLAY = 300, 33                    # two 256-position blocks, the second ragged; 33 layers leave no cloud group empty (asserted below)
_cache = {}


def _kind(rk):
    return "r4" if rk == 4 else "r8"


def all_class_columns(n, nlay, start, aerosol=True):
    """chou_sw_inputs with the clouds of tests/test_gpu_chou.py::test_sorad_all_cloud_group_classes: every one of the eight classes (which
    of the high / middle / low groups hold cloud) populated and interleaved, so that 256-position blocks hold several classes and the
    positions differ from the columns.  The precondition is asserted on the inputs."""
    key = (n, nlay, start, aerosol)
    if key in _cache:
        return _cache[key]
    from geosradiation_gridcomp_amd import synth
    inp = synth.make_columns(n, nlay, start=start, cloudy_frac=1.0, aerosol=True)
    cs = synth.chou_sw_inputs(inp, aerosol=aerosol)
    ict, icb = int(cs["ict"]), int(cs["icb"])
    lev = np.arange(1, nlay + 1)
    grp = np.where(lev < ict, 4, np.where(lev < icb, 2, 1))
    assert all((grp == g).sum() >= 2 for g in (4, 2, 1)), "a cloud group with fewer than two layers"
    cls = np.arange(n) % 8
    fcld = np.array(cs["fcld"], copy=True); cwc = np.array(cs["cwc"], copy=True)
    rng = np.random.default_rng(5)
    for c in range(8):
        cols = np.where(cls == c)[0]
        for g in (4, 2, 1):
            lays = np.where(grp == g)[0]
            if c & g:
                pick = rng.choice(lays, size=2, replace=False)
                fcld[np.ix_(pick, cols)] = rng.uniform(0.2, 0.9, (2, cols.size)).astype(fcld.dtype)
                cwc[:2, pick[:, None], cols[None, :]] = 2.0e-5
            else:
                fcld[np.ix_(lays, cols)] = 0
                cwc[:, lays[:, None], cols[None, :]] = 0
    cs = dict(cs, fcld=fcld, cwc=cwc)
    have = np.array([(4 if (fcld[grp == 4][:, i] > 0).any() else 0) + (2 if (fcld[grp == 2][:, i] > 0).any() else 0) +
                     (1 if (fcld[grp == 1][:, i] > 0).any() else 0) for i in range(n)])
    assert set(have) == set(range(8))
    assert all(len(set(have[b:b + 256])) > 1 for b in range(0, n, 256))          # blocks of columns are not class-homogeneous: the sort has work
    if aerosol:
        assert (cs["taua"] > 0).any() and (cs["ssaa"] > 0).any() and (cs["asya"] != 0).any()
    else:
        assert not cs["taua"].any() and not cs["ssaa"].any() and not cs["asya"].any()
    _cache[key] = cs
    return cs


def without_aerosols(cs):
    z = np.zeros_like(cs["taua"])
    return dict(cs, taua=z, ssaa=z.copy(), asya=z.copy())


def launches(ctx, slot):
    ms = ctypes.c_double(); n = ctypes.c_long()
    ctx._chk(ctx.L.geosrad_profile_read(ctx.h, ctypes.c_int(slot), ctypes.byref(ms), ctypes.byref(n)))
    return n.value


def dev_call(ctx, cs, na=None, counts=None, do_drfband=True, drop=(), expect=0):
    """geosrad_sorad_dev (na None) or geosrad_sorad_na_dev (na = the names of NA to pass; () = all members NULL; "null" = na_out NULL) on
    poisoned outputs.  counts: dict receiving the launches of the preparation and the pass slot.  drop: outputs passed as NULL.
    Returns {name: numpy} of the 13 outputs and the 5 aerosol-free arrays (poison where not written)."""
    import torch
    n1, m = cs["pl"].shape
    tdt = torch.float32 if ctx.dtype == np.float32 else torch.float64
    d = {k: torch.from_numpy(np.ascontiguousarray(cs[k], dtype=ctx.dtype)).cuda() for k in IN}
    shape = lambda k: (n1, m) if TWIN.get(k, k) in PROFILES else ((8, m) if TWIN.get(k, k) in ("flx_sfc_band", "drband", "dfband") else (m,))
    for k in OUT + NA:
        d[k] = torch.full(shape(k), POISON, dtype=tdt, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    ptr = {k: v.data_ptr() for k, v in d.items() if k not in drop}
    args = (st, m, n1 - 1, 8, ptr, cs["co2"], cs["ict"], cs["icb"], cs["hk_uv"], cs["hk_ir"])
    if counts is not None:
        ctx.profile(True)
    try:
        if expect:
            hu = np.ascontiguousarray(cs["hk_uv"], dtype=ctx.dtype); hi = np.ascontiguousarray(cs["hk_ir"], dtype=ctx.dtype)
            v = lambda k: ctypes.c_void_p(ptr[k]) if ptr.get(k) else None
            tab = (ctypes.c_void_p * 5)(*[ptr[k] for k in NA])
            ci = ctypes.c_int
            rc = ctx.L.geosrad_sorad_na_dev(
                ctx.h, ctypes.c_void_p(st), ci(m), ci(n1 - 1), ci(8), *[v(k) for k in IN[:5]], ctypes.c_double(cs["co2"]), v("cwc"), v("fcld"),
                ci(int(cs["ict"])), ci(int(cs["icb"])), v("reff"), hu.ctypes.data_as(ctypes.c_void_p), hi.ctypes.data_as(ctypes.c_void_p),
                *[v(k) for k in IN[8:]], v("flx"), v("flc"), v("fdiruv"), v("fdifuv"), v("fdirpar"), v("fdifpar"), v("fdirir"), v("fdifir"),
                v("flxu"), v("flcu"), v("flx_sfc_band"), ci(1 if do_drfband else 0), v("drband"), v("dfband"), tab)
            assert rc == expect, (rc, ctx.L.geosrad_last_error(ctx.h).decode())
        elif na is None:
            ctx.sorad_dev(*args, do_drfband=do_drfband)
        else:
            ctx.sorad_na_dev(*args, do_drfband=do_drfband, na_ptr=None if na == "null" else {k: d[k].data_ptr() for k in na})
        torch.cuda.synchronize()
        if counts is not None:
            counts["prep"] = launches(ctx, SLOT_PREP); counts["pass"] = launches(ctx, SLOT_PASS)
    finally:
        if counts is not None:
            ctx.profile(False)
    return {k: d[k].cpu().numpy() for k in OUT + NA}


def check_shared_call(ctx, cs):
    """the statement of test 1 for one context: na_out = the context's own sorad_dev without aerosols, out = its sorad_dev with them"""
    g = dev_call(ctx, cs, na=NA)
    w = dev_call(ctx, cs)
    z = dev_call(ctx, without_aerosols(cs))
    for k in NA:
        assert np.array_equal(g[k], z[TWIN[k]]), k
    for k in OUT:
        assert np.array_equal(g[k], w[k]), k
        assert np.isfinite(g[k]).all() and (g[k] != POISON).all(), k
    for k in NA:
        assert np.isfinite(g[k]).all() and (g[k] != POISON).all(), k
        assert (w[k] == POISON).all(), k                       # the plain entry point has no such output
    assert not np.array_equal(g["flx_na"], g["flx"])
    return g


def fresh_context(rk, env=None, overcast=False):
    from geosradiation_gridcomp_amd.api import Context
    old = {k: os.environ.get(k) for k in (env or {})}
    os.environ.update(env or {})
    try:
        ctx = Context(rk)
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v
    if overcast:
        ctx.set_overcast(sorad=True)
    return ctx


@pytest.mark.parametrize("rk", [8, 4])
def test_equals_a_call_without_aerosols(gpu_ctx, rk):
    """300 columns x 33 layers, all eight classes, aerosols on, do_drfband = 1: the five na_out arrays are the bits of sorad_dev with three
    arrays of zeros, the 13 regular outputs the bits of sorad_dev with the aerosols; against the oracle without aerosols within the
    bounds of tests/test_gpu_chou.py::test_sorad_matches_oracle (1e-9 of the insolation in fp64, 2e-5 in fp32)."""
    from oracle import clib
    ctx = gpu_ctx[rk]
    cs = all_class_columns(NCOL, NLAY, 880_000)
    g = check_shared_call(ctx, cs)
    o = clib.sorad(all_class_columns(NCOL, NLAY, 880_000, aerosol=False), _kind(rk), do_drfband=True)
    assert o["rc"] == 0
    tol = 1e-9 if rk == 8 else 2e-5          # test_sorad_matches_oracle's
    for k in NA:
        err = np.abs(g[k].astype(np.float64) - o[TWIN[k]].astype(np.float64)).max()
        print(f"real_kind {rk} {k}: max |gpu - oracle| = {err:.3e} (bound {tol:g})")
        assert err <= tol, k
    # the aerosols of these inputs dim the surface: taking them away is visible well above the bound
    assert np.abs(g["flx_na"][-1].astype(np.float64) - g["flx"][-1]).max() > 100 * tol


@pytest.mark.parametrize("path", ["col", "overcast"])
@pytest.mark.parametrize("rk", [8, 4])
def test_same_on_the_other_two_paths(rk, path):
    """GEOSRAD_SORAD_PATH=col (k_sorad_col, set around geosrad_create only) and GEOSRAD_OVERCAST_SORAD (k_sorad_pass_oc): each compared with
    that same context's own sorad_dev"""
    ctx = fresh_context(rk, env={"GEOSRAD_SORAD_PATH": "col"}) if path == "col" else fresh_context(rk, overcast=True)
    try:
        label = ctx.L.geosrad_kernel_label(ctx.h, ctypes.c_int(SLOT_PASS)).decode()
        assert label == ("k_sorad_col" if path == "col" else "k_sorad_pass_oc")
        check_shared_call(ctx, all_class_columns(NCOL, NLAY, 880_000))
    finally:
        ctx.close()


@pytest.mark.parametrize("rk", [8, 4])
def test_zero_aerosols_are_no_aerosols_and_what_runs(gpu_ctx, rk):
    """With taua = ssaa = asya exact zeros each aerosol-free array equals its twin; the preparation slot counts the same in a plain and in
    an aerosol-free call and the pass slot twice as many; the workspace of an aerosol-free call exceeds that of a plain call by less
    than one pass's scratch planes, 30 (np + 2) m reals: neither scr nor the aerosol planes were duplicated."""
    ctx = gpu_ctx[rk]
    cs = all_class_columns(NCOL, NLAY, 880_000)
    z = dev_call(ctx, without_aerosols(cs), na=NA)
    for k in NA:
        assert np.array_equal(z[k], z[TWIN[k]]), k
    plain, shared = {}, {}
    dev_call(ctx, cs, counts=plain)
    dev_call(ctx, cs, na=NA, counts=shared)
    assert plain["prep"] >= 1 and plain["pass"] >= 1
    assert shared["prep"] == plain["prep"] and shared["pass"] == 2 * plain["pass"], (plain, shared)
    a, b = fresh_context(rk), fresh_context(rk)
    try:
        dev_call(a, cs)
        dev_call(b, cs, na=NA)
        wa, wb = a.workspace_bytes(), b.workspace_bytes()
    finally:
        a.close(); b.close()
    print(f"real_kind {rk}: workspace plain {wa} B, aerosol-free {wb} B, one pass's planes {30 * (NLAY + 2) * NCOL * rk} B")
    assert wa > 0 and 0 <= wb - wa < 30 * (NLAY + 2) * NCOL * rk


@pytest.mark.parametrize("rk", [8, 4])
def test_null_members(gpu_ctx, rk):
    """Only flc_na and flx_sfc_band_na given: those two carry the full call's bits, the other three keep the poison.  na_out all NULL, and
    na_out NULL: the pass slot counts as in the plain call and every regular output is bitwise the plain call's."""
    ctx = gpu_ctx[rk]
    cs = all_class_columns(NCOL, NLAY, 880_000)
    full = dev_call(ctx, cs, na=NA)
    some = dev_call(ctx, cs, na=("flc_na", "flx_sfc_band_na"))
    for k in NA:
        if k in ("flc_na", "flx_sfc_band_na"):
            assert np.array_equal(some[k], full[k]), k
        else:
            assert (some[k] == POISON).all(), k
    for k in OUT:
        assert np.array_equal(some[k], full[k]), k
    cp = {}
    plain = dev_call(ctx, cs, counts=cp)
    for na in ((), "null"):
        cn = {}
        g = dev_call(ctx, cs, na=na, counts=cn)
        assert cn == cp, (na, cn, cp)
        for k in OUT:
            assert np.array_equal(g[k], plain[k]), (na, k)
        for k in NA:
            assert (g[k] == POISON).all(), (na, k)


@pytest.mark.parametrize("rk", [8, 4])
def test_chunking_is_invisible(gpu_ctx, rk):
    """600 columns with geosrad_set_chunk(256) (three chunks, the last ragged) against one chunk"""
    ctx = gpu_ctx[rk]
    cs = all_class_columns(600, NLAY, 881_000)
    one = dev_call(ctx, cs, na=NA)
    ctx.set_chunk(256)
    try:
        cut = dev_call(ctx, cs, na=NA)
        part = dev_call(ctx, cs, na=("flx_na",))          # the members not taken have their place in the workspace, whole call wide
    finally:
        ctx.set_chunk(131072)
    for k in OUT + NA:
        assert np.array_equal(cut[k], one[k]), k
    assert np.array_equal(part["flx_na"], one["flx_na"]) and (part["flc_na"] == POISON).all()
    assert (one["flx_na"] != POISON).all()


@pytest.mark.parametrize("rk", [8, 4])
def test_host_pointers(gpu_ctx, rk):
    """sorad_na_columns at 300 columns with GEOSRAD_HOST_CHUNK = 128 (three host chunks, the last ragged) gives the _dev bits; so does a
    two-shard context; a member not taken is not returned and does not disturb the others"""
    from geosradiation_gridcomp_amd.api import Context
    cs = all_class_columns(NCOL, NLAY, 880_000)
    want = dev_call(gpu_ctx[rk], cs, na=NA)
    one = fresh_context(rk, env={"GEOSRAD_HOST_CHUNK": "128"})
    two = Context(rk, devices=[0, 0])
    try:
        for c in (one, two):
            h = c.sorad_na_columns(cs, do_drfband=True)
            for k in OUT + NA:
                assert np.array_equal(h[k], want[k]), k
        h = one.sorad_na_columns(cs, do_drfband=True, na=("flxu_na",))
        assert np.array_equal(h["flxu_na"], want["flxu_na"]) and "flx_na" not in h
        p = one.sorad_columns(cs, do_drfband=True)
        for k in OUT:
            assert np.array_equal(p[k], want[k]), k
    finally:
        one.close(); two.close()


@pytest.mark.parametrize("rk", [8, 4])
def test_argument_validation_launches_nothing(rk):
    """do_drfband with drband NULL, and tables not loaded: GEOSRAD_EINVAL, the profile slots read 0 and the outputs are still poisoned"""
    from geosradiation_gridcomp_amd.api import Context
    cs = all_class_columns(NCOL, NLAY, 880_000)
    ctx = fresh_context(rk)
    try:
        counts = {}
        g = dev_call(ctx, cs, counts=counts, drop=("drband",), expect=EINVAL)
        assert counts == {"prep": 0, "pass": 0}
        for k in OUT + NA:
            assert (g[k] == POISON).all(), k
    finally:
        ctx.close()
    bare = Context(rk, tables=False)          # a context without the Chou-Suarez SW tables
    try:
        counts = {}
        g = dev_call(bare, cs, counts=counts, expect=EINVAL)
        assert counts == {"prep": 0, "pass": 0}
        for k in OUT + NA:
            assert (g[k] == POISON).all(), k
    finally:
        bare.close()
