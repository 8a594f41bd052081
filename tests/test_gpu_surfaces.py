"""GPU tests (pytest -m gpu) of the surface inputs every other fixture leaves degenerate: a different emissivity in each of the 16
RRTMG_LW bands, four different SW albedos, a tiled and vegetated irrad surface - through every kernel path and entry point that carries
them.  tests/test_oracle_surfaces.py states the identities, shows on the oracle that a swapped map or a shifted band row breaks them in
every column, and holds the helpers used here.

Residuals measured on the MI355X (the oracle's own are in tests/test_oracle_surfaces.py):
  rrtmg_lw against the reference's golden:       fp64 5.7e-13,   fp32 3.7e-4 W m-2 (bounds 1e-6, 2e-3), the three paths alike
  rrtmg_sw surface identities, of the TOA flux:  fp64 1.7e-16,   fp32 7.7e-8   (bounds 1e-12, 1e-5)
  sorad surface identity, of the insolation:     fp64 5.6e-17,   fp32 5.8e-8   (bounds 1e-12, 1e-5)
  irrad mixing property, fp64:                   2.3e-13 W m-2                 (bound 1e-8)"""
import functools
import os

import numpy as np
import pytest

from geosradiation_gridcomp_amd import synth
from tests.conftest import FLUX, load_golden
from tests.test_chou_overcast import ocref          # noqa: F401  (fixture: the OVERCAST restatement of sorad)
from tests.test_gpu_lw import TOL_DFDT, TOL_FLUX
from tests.test_gpu_sw import SFC, SWFLUX, flux_tol
from tests.test_oracle_surfaces import EMIS_GOLDEN, IRRAD_OUT, irrad_mixing_residual, sorad_surface_residual, sw_surface_residuals

pytestmark = pytest.mark.gpu
LW_OUT = FLUX + ("clearCounts", "olrb", "dolrb_dTs")
SO_KEYS = ("flx", "flc", "flxu", "flcu", "fdiruv", "fdifuv", "fdirpar", "fdifpar", "fdirir", "fdifir", "flx_sfc_band", "drband", "dfband")


def _kind(rk):
    return "r4" if rk == 4 else "r8"


def _contexts(var, value):
    """{4: Context(4), 8: Context(8)} created with the environment variable `var` = `value` (None: unset), which geosrad_create reads"""
    from geosradiation_gridcomp_amd.api import Context
    old = os.environ.get(var)
    if value is None:
        os.environ.pop(var, None)
    else:
        os.environ[var] = value
    try:
        return {4: Context(4), 8: Context(8)}
    finally:
        if old is None:
            os.environ.pop(var, None)
        else:
            os.environ[var] = old


@pytest.fixture(scope="module")
def lw_ctxs(gpu_ctx):
    """RRTMG_LW contexts by kernel path: the default band kernels, GEOSRAD_LW_PATH=cols and =split"""
    made = {"cols": _contexts("GEOSRAD_LW_PATH", "cols"), "split": _contexts("GEOSRAD_LW_PATH", "split")}
    yield dict(made, default=gpu_ctx)
    for c in made.values():
        for x in c.values():
            x.close()


@pytest.fixture(scope="module")
def sw_ctxs(gpu_ctx):
    """RRTMG_SW contexts by kernel path: the default sweep and GEOSRAD_SW_PATH=bands"""
    made = _contexts("GEOSRAD_SW_PATH", "bands")
    yield {"default": gpu_ctx, "bands": made}
    for x in made.values():
        x.close()


@pytest.fixture(scope="module")
def sorad_ctxs(gpu_ctx):
    """sorad contexts: the default passes, GEOSRAD_SORAD_PATH=col (on-chip), and contexts of this module's own for the OVERCAST mode"""
    from geosradiation_gridcomp_amd.api import Context
    col = _contexts("GEOSRAD_SORAD_PATH", "col")
    oc = {4: Context(4), 8: Context(8)}
    for c in oc.values():
        c.set_overcast(sorad=True)
    yield {"default": gpu_ctx, "col": col, "overcast": oc}
    for c in (col, oc):
        for x in c.values():
            x.close()


# ==== RRTMG_LW: per-band emissivity, pinned to the reference =====================================================================
@pytest.mark.parametrize("name", EMIS_GOLDEN)
@pytest.mark.parametrize("path", ["default", "cols", "split"])
@pytest.mark.parametrize("rk", [8, 4])
def test_lw_band_emissivity_matches_reference_golden(lw_ctxs, rk, path, name):
    """fluxes, clearCounts and the band outputs of the reference's own Fortran"""
    ctx = lw_ctxs[path][rk]
    inp, g, ih = load_golden(name)
    kind = _kind(rk)
    bo = np.ones(16, dtype=np.int32)
    ctx.set_inhomogeneity(ih)
    try:
        o = ctx.rrtmg_lw_columns(inp, band_output=bo)
    finally:
        ctx.set_inhomogeneity(0)
    for k in FLUX:
        tol = TOL_DFDT[rk] if "dTs" in k else TOL_FLUX[rk]
        err = np.abs(o[k].astype(np.float64) - g[f"{kind}_{k}"].astype(np.float64)).max()
        print(f"{path} rk={rk} {k}: max error {err:.3e} (tol {tol:g})")
        assert err <= tol, (k, err)
    assert np.abs(o["clearCounts"] - g[f"{kind}_clearCounts"]).max() <= (0 if rk == 8 else 1)
    assert np.abs(o["olrb"].astype(np.float64) - g[f"{kind}_olrb"]).max() <= TOL_FLUX[rk]
    assert np.abs(o["dolrb_dTs"].astype(np.float64) - g[f"{kind}_dolrb_dTs"]).max() <= TOL_DFDT[rk]


@functools.lru_cache(maxsize=None)
def lw_ragged_case():
    """(150 columns with per-band emissivities, {kind: oracle fluxes}); the oracle is pinned bit for bit to the reference on the golden
    case of the same kind (tests/test_oracle_surfaces.py)"""
    from oracle import clib
    inp = synth.make_columns(150, 72, start=8900, aerosol=True, cloudy_frac=0.8, emis_bands=True)
    ref = {}
    for kind in ("r8", "r4"):
        clib.set_inhomogeneity(1, kind)
        try:
            ref[kind] = clib.rrtmg_lw(inp, kind, band_output=np.ones(16, dtype=np.int32))
        finally:
            clib.set_inhomogeneity(0, kind)
        assert ref[kind]["rc"] == 0
    # what fp32 costs the reference itself on these columns: its r4 build against its r8 build, clear-sky derivative (no McICA in it)
    ref["own_dfdt"] = float(np.abs(ref["r4"]["duflxc_dTs"].astype(np.float64) - ref["r8"]["duflxc_dTs"]).max())
    return inp, ref


@pytest.mark.parametrize("path", ["default", "cols", "split"])
@pytest.mark.parametrize("rk", [8, 4])
def test_lw_band_emissivity_through_ragged_chunks(lw_ctxs, rk, path):
    """150 columns in chunks of 64 + 64 + 22 (64 is the smallest chunk geosrad_set_chunk takes, so the 16 golden columns cannot be
    cut): the 16 emis rows of the staging pipeline from a non-zero first column on - the bits of the one-chunk call, which agrees with
    the oracle.  fp32 derivatives: on these columns the reference's own r4 build is 4.4e-5 W m-2 K-1 from its r8 build (1.2e-5 on the
    columns tests/test_gpu_lw.py took TOL_DFDT from), so the bound is the larger of TOL_DFDT and that distance, computed from the oracle
    pair here; the fluxes and fp64 keep the tolerances of tests/test_gpu_lw.py."""
    ctx = lw_ctxs[path][rk]
    inp, ref = lw_ragged_case()
    r = ref[_kind(rk)]
    bo = np.ones(16, dtype=np.int32)
    ctx.set_inhomogeneity(1)
    try:
        o = ctx.rrtmg_lw_columns(inp, band_output=bo)
        ctx.set_chunk(64)
        c = ctx.rrtmg_lw_columns(inp, band_output=bo)
    finally:
        ctx.set_chunk(131072)
        ctx.set_inhomogeneity(0)
    for k in LW_OUT:
        np.testing.assert_array_equal(c[k], o[k], err_msg=k)
    tol_dfdt = TOL_DFDT[8] if rk == 8 else max(TOL_DFDT[4], ref["own_dfdt"])
    for k in FLUX + ("olrb", "dolrb_dTs"):
        tol = tol_dfdt if "dTs" in k else TOL_FLUX[rk]
        err = np.abs(o[k].astype(np.float64) - r[k].astype(np.float64)).max()
        assert err <= tol, (k, err, tol)
    assert np.abs(o["clearCounts"] - r["clearCounts"]).max() <= (0 if rk == 8 else 1)


@pytest.mark.parametrize("rk", [8, 4])
def test_lw_band_emissivity_through_dev_and_na_entries(gpu_ctx, rk):
    """geosrad_rrtmg_lw_dev and geosrad_rrtmg_lw_na[_dev] on the same columns: the host entry's bits; the aerosol-laden half of _na is
    the plain call (tests/test_gpu_lw_na.py says so for emis = 0.98), and its aerosol-free half differs"""
    import torch
    from tests.test_gpu_lw_na import NA, NAMES, lw_dev
    ctx = gpu_ctx[rk]
    inp, _, ih = load_golden(EMIS_GOLDEN[0])
    nlay, ncol = inp["play"].shape
    bo = np.ones(16, dtype=np.int32)
    ctx.set_inhomogeneity(ih)
    try:
        h = ctx.rrtmg_lw_columns(inp, band_output=bo)
        hn = ctx.rrtmg_lw_na_columns(inp, band_output=bo)
        dn = lw_dev(ctx, inp, "na")
        t = {k: torch.from_numpy(np.ascontiguousarray(inp[k], dtype=ctx.dtype)).cuda() for k in NAMES + ["tauaer"]}
        tdt = t["play"].dtype
        for k in FLUX:
            t[k] = torch.full((nlay + 1, ncol), -7.0, dtype=tdt, device="cuda")
        for k in ("olrb", "dolrb_dTs"):
            t[k] = torch.full((ncol, 16), -7.0, dtype=tdt, device="cuda")
        t["clearCounts"] = torch.zeros((4, ncol), dtype=torch.int32, device="cuda")
        st = torch.cuda.current_stream().cuda_stream
        ctx.rrtmg_lw_dev(st, ncol, nlay, True, {k: v.data_ptr() for k, v in t.items()}, 3, 1, int(inp["dyofyr"]), int(inp["cloudLM"]),
                         int(inp["cloudMH"]), band_output=bo)
        ctx.check(st)
    finally:
        ctx.set_inhomogeneity(0)
    for k in LW_OUT:
        np.testing.assert_array_equal(t[k].cpu().numpy(), h[k], err_msg=k)
        np.testing.assert_array_equal(hn[k], h[k], err_msg=k)
    for k in FLUX + NA + ("clearCounts",):
        np.testing.assert_array_equal(dn[k], hn[k], err_msg=k)
    assert np.isfinite(hn["uflx_na"]).all() and not np.array_equal(hn["dflx_na"], hn["dflx"])


# ==== RRTMG_SW: four different albedos ===========================================================================================
@functools.lru_cache(maxsize=None)
def sw_case(ncol, nlay, normFlx):
    """(columns, {kind: oracle result}): computed once, shared, never modified"""
    from oracle import clib
    inp = synth.make_columns(ncol, nlay, start=6100, aerosol=True, cloudy_frac=0.6, distinct_albedos=True)
    ref = {}
    for kind in ("r8", "r4"):
        clib.set_inhomogeneity(1, kind)
        try:
            ref[kind] = clib.rrtmg_sw(inp, prec=kind, iaer=10, normFlx=normFlx, do_drfband=True)
        finally:
            clib.set_inhomogeneity(0, kind)
        assert ref[kind]["rc"] == 0
    return inp, ref


def check_sw(ctx, rk, ncol, nlay, normFlx, tag, chunk=None):
    inp, ref = sw_case(ncol, nlay, normFlx)
    o = ref[_kind(rk)]
    ctx.set_inhomogeneity(1)
    try:
        g = ctx.rrtmg_sw_columns(inp, iaer=10, normFlx=normFlx, do_drfband=True)
        if chunk:
            ctx.set_chunk(chunk)
            c = ctx.rrtmg_sw_columns(inp, iaer=10, normFlx=normFlx, do_drfband=True)
    finally:
        ctx.set_chunk(131072)
        ctx.set_inhomogeneity(0)
    # the surface identities on the GPU's own outputs, every column
    net, up = sw_surface_residuals(g, inp, nlay)
    print(f"{tag} rk={rk} {ncol} x {nlay} normFlx={normFlx}: surface identity residuals / TOA: net {net.max():.2e}, upward {up.max():.2e}")
    bound = 1e-12 if rk == 8 else 1e-5
    assert net.max() <= bound and up.max() <= bound, (net.max(), up.max())
    # the oracle: tolerance and column policy of tests/test_gpu_sw.py::test_sw_fluxes_match_oracle
    if rk == 8:
        np.testing.assert_array_equal(g["clearCounts"], o["clearCounts"])
        same = np.ones(ncol, dtype=bool)
    else:
        same = (g["clearCounts"] == o["clearCounts"]).all(axis=0)
        assert same.mean() >= 0.95
    tol = flux_tol(rk, o["swdflx"][nlay])
    for k in SWFLUX + SFC + ("drband", "dfband"):
        err = (np.abs(g[k].astype(np.float64) - o[k].astype(np.float64)) / tol)[..., same]
        worst = err.reshape(-1, err.shape[-1]).max(axis=0)
        if rk == 8:
            assert worst.max() <= 1.0, (k, worst.max())
        else:
            assert worst.max() <= 10.0 and (worst > 1.0).mean() <= 0.01, (k, worst.max(), (worst > 1.0).mean())
    if chunk:
        for k in SWFLUX + SFC + ("drband", "dfband", "clearCounts"):
            np.testing.assert_array_equal(c[k], g[k], err_msg=k)


@pytest.mark.parametrize("path", ["default", "bands"])
@pytest.mark.parametrize("rk", [8, 4])
def test_sw_distinct_albedos_surface_identities_and_oracle(sw_ctxs, rk, path):
    """96 x 72 cloudy and clear columns with aerosols; chunks of 64 + 32 columns (64 is the smallest chunk geosrad_set_chunk takes) give
    the same bits"""
    check_sw(sw_ctxs[path][rk], rk, 96, 72, 0, path, chunk=64)


@pytest.mark.parametrize("path", ["default", "bands"])
@pytest.mark.parametrize("rk", [8, 4])
@pytest.mark.parametrize("ncol,nlay,normFlx", [(7, 137, 0), (96, 72, 1)])
def test_sw_distinct_albedos_137_layers_and_normalised(sw_ctxs, rk, path, ncol, nlay, normFlx):
    check_sw(sw_ctxs[path][rk], rk, ncol, nlay, normFlx, path)


# ==== sorad: four different albedos ==============================================================================================
@functools.lru_cache(maxsize=None)
def sorad_inputs():
    inp = synth.make_columns(48, 72, start=6300, aerosol=True, cloudy_frac=0.7, distinct_albedos=True)
    return synth.chou_sw_inputs(inp, aerosol=True)


@pytest.mark.parametrize("path", ["default", "col", "overcast"])
@pytest.mark.parametrize("rk", [8, 4])
def test_sorad_distinct_albedos_surface_identity_and_oracle(sorad_ctxs, ocref, rk, path):  # noqa: F811
    from oracle import clib
    cs = sorad_inputs()
    g = sorad_ctxs[path][rk].sorad_columns(cs, do_drfband=True)
    res = sorad_surface_residual(g, cs)
    print(f"sorad {path} rk={rk}: surface identity residual {res.max():.2e}")
    assert res.max() <= (1e-12 if rk == 8 else 1e-5), res.max()
    o = ocref.sorad(cs, _kind(rk)) if path == "overcast" else clib.sorad(cs, _kind(rk), do_drfband=True)
    assert o["rc"] == 0
    tol = 1e-9 if rk == 8 else 2e-5          # the bounds of tests/test_gpu_chou.py::test_sorad_matches_oracle
    for k in SO_KEYS:
        assert np.abs(g[k].astype(np.float64) - o[k].astype(np.float64)).max() <= tol, k


# ==== irrad: tiled and vegetated surfaces ========================================================================================
@functools.lru_cache(maxsize=None)
def irrad_inputs(ns, vegetated, ncol, nlay):
    inp = synth.make_columns(ncol, nlay, start=6500, aerosol=True, cloudy_frac=0.7)
    return synth.chou_lw_inputs(inp, aerosol=True, ns=ns, vegetated=vegetated)


@pytest.mark.parametrize("ncol,nlay", [(48, 72), (65, 33), (150, 33)])
@pytest.mark.parametrize("ns,vegetated", [(2, True), (3, True), (3, False)])
@pytest.mark.parametrize("rk", [8, 4])
def test_irrad_tiled_surfaces_match_oracle(gpu_ctx, rk, ns, vegetated, ncol, nlay):
    """sfcflux's loop over sub-surfaces with and without vegetation against the oracle (the bounds of
    tests/test_gpu_chou.py::test_irrad_matches_oracle); with chunks of 64 columns, the smallest geosrad_set_chunk takes (65 = 64 + 1,
    150 = 64 + 64 + 22: the ns and 10 ns row staging shapes from a non-zero first column on), the same bits"""
    from oracle import clib
    ctx = gpu_ctx[rk]
    ch = irrad_inputs(ns, vegetated, ncol, nlay)
    try:
        g = ctx.irrad_columns(ch)
        ctx.set_chunk(64)
        c = ctx.irrad_columns(ch)
    finally:
        ctx.set_chunk(131072)
    o = clib.irrad(ch, _kind(rk))
    assert o["rc"] == 0
    tol = 1e-6 if rk == 8 else 2e-2
    for k in IRRAD_OUT:
        t = (1e-8 if rk == 8 else 2e-4) if k == "dfdts" else tol
        err = np.abs(g[k].astype(np.float64) - o[k].astype(np.float64)).max()
        assert err <= t, (k, err)
    for k in IRRAD_OUT + ("taudiag",):
        np.testing.assert_array_equal(c[k], g[k], err_msg=k)


@pytest.mark.parametrize("ns,vegetated", [(2, True), (3, True)])
def test_irrad_tiles_mix_linearly_on_the_gpu(gpu_ctx, ns, vegetated):
    """the GPU's own outputs in fp64: the tiled call is the fs-weighted sum of its sub-surfaces run alone (fp32 is held through the oracle)"""
    ch = irrad_inputs(ns, vegetated, 48, 72)
    res = irrad_mixing_residual(gpu_ctx[8].irrad_columns, ch)
    print(f"irrad GPU fp64 ns={ns}: mixing residual {res:.2e} W m-2")
    assert res <= 1e-8, res


@pytest.mark.parametrize("rk", [8, 4])
def test_irrad_tiled_surface_through_a_multi_device_context(gpu_ctx, rk):
    """ns = 2 through geosrad_create_multi with device_ids = {0, 0}: two shards of 24 columns, the second at a column offset inside every
    (ns, m) and (10, ns, m) array - the single-device bits"""
    from geosradiation_gridcomp_amd.api import Context
    ch = irrad_inputs(2, True, 48, 72)
    a = gpu_ctx[rk].irrad_columns(ch)
    two = Context(rk, devices=[0, 0])
    try:
        b = two.irrad_columns(ch)
    finally:
        two.close()
    for k in IRRAD_OUT + ("taudiag",):
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)
