"""GPU tests of the RRTMG front ends (rrtmg_front in geosrad.hip): the reference's input assertions where they are made now - the
per-layer ones in k_setcoef / k_sw_setcoef, the aerosol ones in the band kernels, the per-column ones in the slim column pass - and
the multi-block stable partition of the columns into cloud-free | cloudy."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests.conftest import ROOT, FLUX

pytestmark = pytest.mark.gpu

SW_OUT = ("swuflx", "swdflx", "swuflxc", "swdflxc", "nirr", "nirf", "parr", "parf", "uvrr", "uvrf", "fswband")
CLOUDY_EVERY = 3          # columns 0, 3, 6, ... of assertion_columns carry a cloud


def with_clouds(inp, cloudy):
    """`inp` (cloud-free make_columns) with a liquid cloud in layer 1 of the columns where `cloudy` is set, whatever the layer count"""
    out = dict(inp)
    c = np.asarray(cloudy, dtype=bool)
    for k, v in (("cldf", 0.5), ("clwp", 40.0)):
        a = inp[k].copy(); a[1, c] = v; out[k] = a
    return out


def assertion_columns(ncol, nlay):
    from geosradiation_gridcomp_amd import synth
    return with_clouds(synth.make_columns(ncol, nlay, start=1234, aerosol=True), np.arange(ncol) % CLOUDY_EVERY == 0)


def assertion_cases(ncol, nlay):
    """(solver, array, index, value, message; None = the call passes): one negative value per family.  The messages are those of the
    reference's assertions as geosrad_check words them; plev and tlev share a bit in RRTMG_LW, whose message names plev; RRTMG_SW
    asserts tauaer and ssaaer (one message), not asmaer (SW/rrtmg_sw_rad.F90:380-383).  The gas is barely negative, so that no
    table index formed from it downstream leaves its table."""
    clear, cloudy = ncol - 2, ncol - 3 - (ncol - 3) % CLOUDY_EVERY          # (a column of the last 256-column block each)
    assert clear % CLOUDY_EVERY != 0 and cloudy % CLOUDY_EVERY == 0 and cloudy >= 256
    top = nlay - 1
    neg = "negative values in input: "
    cases = []
    for col in (clear, cloudy):
        cases += [("lw", "o3vmr", (top // 2, col), -1e-30, neg + "o3vmr"), ("sw", "o3vmr", (top // 2, col), -1e-30, neg + "o3vmr"),
                  ("lw", "tlay", (3, col), -1.0, neg + "tlay"), ("sw", "tlay", (3, col), -1.0, neg + "tlay"),
                  ("lw", "tlev", (nlay, col), -1.0, neg + "plev"),
                  ("lw", "rei", (1, col), -1.0, neg + "rei"), ("sw", "rei", (1, col), -1.0, neg + "rei"),
                  ("lw", "tauaer", (15, top, col), -1e-4, neg + "tauaer"),
                  ("sw", "tauaer_sw", (13, 0, col), -1e-4, neg + "aerosol optical properties"),
                  ("sw", "ssaaer_sw", (13, 0, col), -1e-4, neg + "aerosol optical properties"),
                  ("sw", "asmaer_sw", (13, 0, col), -1e-4, None)]
    return cases


def run_assertions(ctxs=None):
    """300 columns x 8 and x 33 layers, fp32 and fp64: every case of assertion_cases raises its message, and a clean call passes
    afterwards.  ctxs = None: contexts of this process's own (the child processes of the kernel-path tests)."""
    from geosradiation_gridcomp_amd.api import Context, GeosradInputError
    own = ctxs is None
    if own:
        ctxs = {4: Context(4), 8: Context(8)}
    ncol = 300
    try:
        for nlay in (8, 33):
            inp = assertion_columns(ncol, nlay)
            call = {"lw": lambda c, x: c.rrtmg_lw_columns(x), "sw": lambda c, x: c.rrtmg_sw_columns(x, iaer=10)}
            for rk in (4, 8):
                ctx = ctxs[rk]
                for solver, key, idx, val, msg in assertion_cases(ncol, nlay):
                    bad = dict(inp); bad[key] = inp[key].copy(); bad[key][idx] = val
                    what = (rk, nlay, solver, key, idx)
                    if msg is None:
                        call[solver](ctx, bad)
                        continue
                    try:
                        call[solver](ctx, bad)
                    except GeosradInputError as e:
                        assert msg in str(e), (what, str(e))
                    else:
                        raise AssertionError("no error raised: %r" % (what,))
                o = ctx.rrtmg_lw_columns(inp); s = ctx.rrtmg_sw_columns(inp, iaer=10)
                assert np.isfinite(o["uflx"]).all() and np.isfinite(s["swuflx"]).all()
                for cc, ng in ((o["clearCounts"], 140), (s["clearCounts"], 112)):      # cloud-free columns: every sub-column clear
                    assert np.array_equal((cc == ng).all(axis=0), np.arange(ncol) % CLOUDY_EVERY != 0)
    finally:
        if own:
            for c in ctxs.values():
                c.close()


def test_assertions_survive_the_move(gpu_ctx):
    run_assertions(gpu_ctx)


@pytest.mark.parametrize("var,path", [("GEOSRAD_SW_PATH", "bands"), ("GEOSRAD_LW_PATH", "cols"), ("GEOSRAD_LW_PATH", "split")])
def test_assertions_on_the_other_kernel_paths(var, path):
    """the same through the first RRTMG_SW mapping (k_sw_bands) and the other RRTMG_LW band sweeps (k_lw_cols; k_lw_cells), which make
    the aerosol assertions themselves: a child process each, the path being read from the environment"""
    env = dict(os.environ)
    env.pop("GEOSRAD_SW_PATH", None); env.pop("GEOSRAD_LW_PATH", None)
    env[var] = path
    flags = ["-s"] if sys.flags.no_user_site else []
    r = subprocess.run([sys.executable, *flags, "-c", "import tests.test_gpu_front as t; t.run_assertions(); print('assertions ok')"],
                       cwd=ROOT, env=env, capture_output=True, text=True)
    assert r.returncode == 0 and "assertions ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


PATTERNS = {"none": lambda n: np.zeros(n, bool), "all": lambda n: np.ones(n, bool), "alternating": lambda n: np.arange(n) % 2 == 1,
            "last": lambda n: np.arange(n) == n - 1}


@pytest.mark.parametrize("ncol", [1, 255, 256, 257, 1025, 2500])
def test_partition_multi_block_equals_single_block(gpu_ctx, ncol):
    """all LW and SW outputs and clearCounts of one call are the bits of the same call walked in chunks of 64 columns: a chunk's
    partition is one block (no tile counts), the whole call's one block per 1024 columns from 1025 columns on"""
    from geosradiation_gridcomp_amd import synth
    ctx = gpu_ctx[4]
    base = synth.make_columns(ncol, 8, start=77, aerosol=True)
    for name, pat in PATTERNS.items():
        cloudy = pat(ncol)
        inp = with_clouds(base, cloudy)
        try:
            whole = (ctx.rrtmg_lw_columns(inp), ctx.rrtmg_sw_columns(inp, iaer=10))
            ctx.set_chunk(64)
            chunked = (ctx.rrtmg_lw_columns(inp), ctx.rrtmg_sw_columns(inp, iaer=10))
        finally:
            ctx.set_chunk(131072)
        for w, c, keys, ng in ((whole[0], chunked[0], FLUX, 140), (whole[1], chunked[1], SW_OUT, 112)):
            for k in keys + ("clearCounts",):
                assert np.array_equal(w[k], c[k]), (name, k)
            # the flag a column was partitioned by: cloud-free columns count every sub-column clear
            assert np.array_equal((w["clearCounts"] == ng).all(axis=0), ~cloudy), name
            assert np.isfinite(w[keys[0]]).all()
        if cloudy.any():
            assert not np.array_equal(whole[0]["uflx"][:, cloudy], whole[0]["uflxc"][:, cloudy]), name


def test_rats_call_with_two_gases_equals_separate_calls(gpu_ctx):
    """the RATS passes launch k_setcoef once more per gas, without the assertions: their fluxes are still those of separate calls with
    the gas removed, and the main pass's those of a plain call"""
    from geosradiation_gridcomp_amd import gridcomp as G
    from tests.test_gpu_lw import rats_dev, ragged_columns
    ctx = gpu_ctx[4]
    inp = ragged_columns()
    gases = ["H2O", "CO2"]
    got = rats_dev(ctx, inp, gases, 131072)
    full = ctx.rrtmg_lw_columns(inp)
    for k in FLUX + ("clearCounts",):
        assert np.array_equal(got[k], full[k]), k
    for r, gas in enumerate(gases):
        z = dict(inp); z[G.RAT_VMR[gas]] = np.zeros_like(inp[G.RAT_VMR[gas]])
        sep = ctx.rrtmg_lw_columns(z)
        for k in ("uflx", "dflx", "duflx_dTs"):
            assert np.array_equal(got[k + "_rat"][r], sep[k]), (gas, k)
        assert not np.array_equal(sep["uflx"], full["uflx"]), gas
