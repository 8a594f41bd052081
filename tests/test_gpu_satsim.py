"""GPU (pytest -m gpu): the satellite simulator's ISCCP path of include/geosrad_satsim.h - geosrad_scops, geosrad_icarus, their `_dev`
variants, geosrad_cosp_seeds_dev and geosrad_isccp_dev - in an fp32 context against what the reference's r4 build wrote into
tests/golden/satsim_isccp_72.npz and in an fp64 context against its r8 build; for the shapes the fixture does not hold against the numpy
restatement that tests/test_satsim_oracle.py pins to the same fixture.

Bounds (the issue's).  SCOPS: mask and final seeds bit for bit.  ICARUS histogram bins: fp64 no sub-column in another bin; fp32 at most
0.2 % of the batch's cloudy sub-columns (a cap: the reference's own two builds move none).  Continuous outputs: fp32 at most 4 x the
fixture's spread_* (the reference's own r4-against-r8 difference of that output; the device's exp / log differ from libm's by a few ulp,
the order of r4 rounding itself); fp64 the larger of 64 eps relative (the rule of tests/test_sw_clouds.py for chains through log) and 4 x
what the float64 restatement differs from the r8 fixture (restate64rel_*, measured on the CPU, in the fixture).  -1.E+30 exactly wherever the
reference leaves it.  Every comparison prints its measured figure (pytest -s); DESIGN.md 4.12 keeps them.

The chunked host variants: geosrad_set_chunk refuses fewer than 64 columns, so the three chunks are those of the batch taken twice
(192 points, chunks of 64: a chunk boundary inside each copy), and the batch itself goes as 64 + 32."""
import numpy as np
import pytest

from tests import satsim_util as U

KINDS = [(4, "r4", np.float32), (8, "r8", np.float64)]
CANARY = -7.0
NCOL = 30


@pytest.fixture(scope="module")
def fx():
    f = np.load(U.FIXTURE)
    return {k: f[k] for k in f.files}


def _batch(fx):
    return {k[3:]: fx[k] for k in fx if k.startswith("in_") and k != "in_emsfc_lw"}


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def _dev(a, dt):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).cuda()


def dev_scops(ctx, seed, cc, conv, overlap, ncol):
    """geosrad_scops_dev: (mask uint8 (nlev, ncol, npoints), seeds after)"""
    import torch
    nlev, npts = cc.shape
    t = {"seed": _dev(seed, np.int32), "cc": _dev(cc, ctx.dtype), "conv": _dev(conv, ctx.dtype),
         "frac_out_u8": torch.full((nlev, ncol, npts), 9, dtype=torch.uint8, device="cuda")}
    try:
        ctx.scops_dev(_stream(), npts, nlev, ncol, {k: v.data_ptr() for k, v in t.items()}, overlap)
        ctx.check(_stream())
    finally:
        torch.cuda.synchronize()
    return t["frac_out_u8"].cpu().numpy(), t["seed"].cpu().numpy()


def _out_tensors(dt, npts, ncol):
    import torch
    shapes = {"fq_isccp": (7, 7, npts), "boxtau": (ncol, npts), "boxptop": (ncol, npts)}
    return {k: torch.full(shapes.get(k, (npts,)), CANARY, dtype=dt, device="cuda") for k in U.ICARUS_OUT}


def dev_icarus(ctx, b, mask, th, thd, want=U.ICARUS_OUT, overlap=3, check=True):
    """geosrad_icarus_dev on device copies of the batch; every output is allocated and canary-filled, those in `want` are passed"""
    import torch
    nlev, npts = b["pfull"].shape
    ncol = mask.shape[1]
    t = {k: _dev(b[k], ctx.dtype) for k in U.IN_2D + ["skt"]}
    t["sunlit"] = _dev(b["sunlit"], np.int32)
    t["frac_out_u8"] = _dev(mask, np.uint8)
    o = _out_tensors(t["skt"].dtype, npts, ncol)
    ptr = {k: v.data_ptr() for k, v in t.items()}
    ptr.update({k: o[k].data_ptr() for k in want})
    try:
        ctx.icarus_dev(_stream(), npts, nlev, ncol, ptr, th, thd, overlap, U.EMSFC_LW)
        if check:
            ctx.check(_stream())
    finally:
        torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in o.items()}


# ---- SCOPS -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("rk,kind,dt", KINDS)
@pytest.mark.parametrize("overlap", [1, 2, 3])
def test_scops_is_the_references_bit_for_bit(gpu_ctx, fx, rk, kind, dt, overlap):
    mask, seed = dev_scops(gpu_ctx[rk], fx["in_seed"], fx["in_cc"], fx["in_conv"], overlap, NCOL)
    np.testing.assert_array_equal(mask, fx[f"mask_ov{overlap}"])
    np.testing.assert_array_equal(seed, fx[f"{kind}_seed_ov{overlap}"])


@pytest.mark.gpu
@pytest.mark.parametrize("rk,kind,dt", KINDS)
@pytest.mark.parametrize("npts,ncol", [(70, 30), (96, 1), (96, 7), (300, 30)])
def test_scops_other_shapes_against_the_restatement(gpu_ctx, rk, kind, dt, npts, ncol):
    """a partial wavefront of points, one and seven sub-columns, more than one block of points; seeds over the whole 32-bit range (the
    first step of a stream is the only one whose state may exceed 2^30), zero among them"""
    b = U.make_batch(npts, 24, seed=77 + npts)
    seed = b["seed"].copy()
    seed[:8] = [0, -1, 2 ** 31 - 1, -2 ** 31, 2 ** 30, -2 ** 30, 1565358, -7]
    for overlap in (1, 2, 3):
        mask, after = dev_scops(gpu_ctx[rk], seed, b["cc"], b["conv"], overlap, ncol)
        rm, rs = U.scops(seed, b["cc"], b["conv"], overlap, ncol, dt)
        np.testing.assert_array_equal(mask, rm, err_msg=f"overlap {overlap}")
        np.testing.assert_array_equal(after, rs, err_msg=f"overlap {overlap}")
        assert (rm > 0).any()


# ---- ICARUS ----------------------------------------------------------------------------------------------------------------------------
def check_icarus(got, fx, kind, dt, s, tag, spread_factor=4.0):
    eps = float(np.finfo(dt).eps)
    miss = dt(U.MISSING)
    ref = {n: fx[f"{kind}_{n}{s}"] for n in U.ICARUS_OUT}
    gb, rb = U.bins_of(got["boxtau"], got["boxptop"]), U.bins_of(ref["boxtau"], ref["boxptop"])
    cloudy = int((rb[0] > 0).sum())
    moved = int(((gb[0] != rb[0]) | (gb[1] != rb[1])).sum())
    print(f"{tag}: {moved} of {cloudy} cloudy sub-columns in another bin")
    assert moved <= (0.002 * cloudy if dt is np.float32 else 0), (tag, moved, cloudy)
    for n in U.ICARUS_OUT:
        g, r = got[n], ref[n]
        assert g.dtype == r.dtype == dt and g.shape == r.shape, (tag, n)
        assert np.array_equal(g == miss, r == miss), (tag, n, "missing values")
    # the histogram: the same cells, each count an exact number of boxarea additions - it differs only where a sub-column moved
    dfq = np.abs(got["fq_isccp"].astype(np.float64) - ref["fq_isccp"].astype(np.float64))
    dfq[ref["fq_isccp"] == miss] = 0
    assert (dfq > 0).sum() <= 2 * moved and dfq.max(initial=0) <= (moved + 0.5) / got["boxtau"].shape[0], (tag, "fq_isccp")
    for n in U.CONTINUOUS:
        g, r = got[n].astype(np.float64), ref[n].astype(np.float64)
        ok = ref[n] != miss
        if not ok.any():
            continue
        d = np.abs(g - r)[ok]
        if dt is np.float32:
            bound = spread_factor * float(fx["spread_" + n + s])
            print(f"{tag} {n}: max |dev - ref| = {d.max():.3e}, {d.max() / max(bound / spread_factor, 1e-300):.2f} x the reference's r4-r8 spread")
            assert d.max() <= bound, (tag, n, float(d.max()), bound)
        else:
            rel = max(64 * eps, 4 * float(fx["restate64rel_" + n + s]))
            e = d / np.maximum(np.abs(r[ok]), 1e-300)
            e[d == 0] = 0
            print(f"{tag} {n}: max rel = {e.max():.3e} = {e.max() / eps:.1f} eps (bound {rel / eps:.0f} eps)")
            assert (d <= rel * np.abs(r[ok])).all(), (tag, n, float(e.max()))


@pytest.fixture(scope="module")
def icarus_runs(gpu_ctx, fx):
    """every (kind, top_height, direction) once, all outputs, shared by the tests below"""
    b = _batch(fx)
    return {(rk, th, thd): dev_icarus(gpu_ctx[rk], b, fx["mask_ov3"], th, thd) for rk, _, _ in KINDS for th, thd in U.OPTION_PAIRS}


@pytest.mark.gpu
@pytest.mark.parametrize("rk,kind,dt", KINDS)
@pytest.mark.parametrize("th,thd", U.OPTION_PAIRS)
def test_icarus_against_the_reference(icarus_runs, fx, rk, kind, dt, th, thd):
    got = icarus_runs[(rk, th, thd)]
    check_icarus(got, fx, kind, dt, f"_th{th}_d{thd}", f"{kind} top_height {th} direction {thd}")
    miss = dt(U.MISSING)
    dark = fx["in_sunlit"] == 0
    if th in (1, 2):
        for n in ("fq_isccp", "totalcldarea", "meanptop", "meantaucld", "meanalbedocld", "boxtau", "boxptop"):
            assert (got[n][..., dark] == miss).all(), n
    if th == 2:
        assert (got["meantb"] == miss).all() and (got["meantbclr"] == miss).all()
    else:
        assert (got["meantb"] > 150).all() and (got["meantbclr"] > 150).all()
    clear = fx["in_cc"].max(axis=0) == 0
    assert (got["boxtau"][:, clear] == miss).all() and (got["boxptop"][:, clear] == miss).all()
    assert ((got["boxtau"] == miss) == (got["boxptop"] == miss)).all()


@pytest.mark.gpu
@pytest.mark.parametrize("rk,kind,dt", KINDS)
@pytest.mark.parametrize("th,thd", U.OPTION_PAIRS)
def test_icarus_identities(icarus_runs, fx, rk, kind, dt, th, thd):
    """oracle-free: the histogram holds every cloudy sub-column once; its part with itau >= 2 is totalcldarea"""
    got = icarus_runs[(rk, th, thd)]
    miss = dt(U.MISSING)
    seen = got["totalcldarea"] != miss
    assert seen.sum() == (96 if th == 3 else 72)
    fq = got["fq_isccp"][:, :, seen].astype(np.float64)
    cloudy = (got["boxtau"][:, seen] != miss).sum(axis=0)
    np.testing.assert_array_equal(np.rint(fq.sum(axis=(0, 1)) * NCOL).astype(np.int64), cloudy)
    assert np.abs(fq.sum(axis=(0, 1)) * NCOL - cloudy).max() <= NCOL * NCOL * float(np.finfo(dt).eps)
    thick = fq[:, 1:, :].sum(axis=(0, 1))
    assert np.abs(thick - got["totalcldarea"][seen]).max() <= NCOL * float(np.finfo(dt).eps)
    assert (cloudy > 0).sum() > 50


@pytest.mark.gpu
@pytest.mark.parametrize("rk,kind,dt", KINDS)
def test_a_null_output_changes_no_other_outputs_bits(gpu_ctx, icarus_runs, fx, rk, kind, dt):
    b = _batch(fx)
    full = icarus_runs[(rk, 1, 2)]
    for drop in (("fq_isccp",), ("boxtau", "boxptop"), ("meantb", "meantbclr", "totalcldarea"), ("meanptop", "meantaucld", "meanalbedocld")):
        got = dev_icarus(gpu_ctx[rk], b, fx["mask_ov3"], 1, 2, want=[n for n in U.ICARUS_OUT if n not in drop])
        for n in U.ICARUS_OUT:
            if n in drop:
                assert (got[n] == dt(CANARY)).all(), n      # nothing was written behind a NULL
            else:
                np.testing.assert_array_equal(got[n], full[n], err_msg=f"{n} without {drop}")


@pytest.mark.gpu
@pytest.mark.parametrize("rk,kind,dt", KINDS)
def test_out_of_range_input_is_an_input_error(gpu_ctx, fx, rk, kind, dt):
    from geosradiation_gridcomp_amd.api import GeosradInputError
    b = _batch(fx)
    b["dem_s"] = b["dem_s"].copy()
    b["dem_s"][40, 17] = 1.5
    with pytest.raises(GeosradInputError, match="dem_s") as e:
        dev_icarus(gpu_ctx[rk], b, fx["mask_ov3"], 1, 2)
    assert e.value.rc == 5
    gpu_ctx[rk].check(_stream())                        # reported once; the flag is down again
    b = _batch(fx)
    b["dtau_c"] = b["dtau_c"].copy(); b["dtau_c"][3, 95] = -1e-3
    nlev, npts = b["pfull"].shape
    mask = np.asarray(fx["mask_ov3"], dtype=dt)
    with pytest.raises(GeosradInputError, match="dtau_c"):      # the host variant returns it itself
        gpu_ctx[rk].icarus(npts, b["sunlit"], nlev, NCOL, b["pfull"], b["phalf"], b["qv"], b["cc"], b["conv"], b["dtau_s"], b["dtau_c"], 1, 2, 3,
                           mask, b["skt"], U.EMSFC_LW, b["at"], b["dem_s"], b["dem_c"])
    dev_icarus(gpu_ctx[rk], _batch(fx), fx["mask_ov3"], 3, 1)      # and a good call after it passes


@pytest.mark.gpu
def test_invalid_options_are_refused(gpu_ctx, fx):
    from geosradiation_gridcomp_amd.api import GeosradError
    ctx = gpu_ctx[4]
    b = _batch(fx)
    small = {k: (v[:4] if v.ndim == 2 else v) for k, v in b.items()}
    small["phalf"] = b["phalf"][:5]
    m = fx["mask_ov3"][:4]
    for kw, what in ((dict(th=0), "top_height"), (dict(th=4), "top_height"), (dict(thd=0), "top_height_direction"), (dict(thd=3), "top_height_direction"),
                     (dict(overlap=0), "overlap"), (dict(overlap=4), "overlap")):
        a = dict(th=1, thd=2, overlap=3); a.update(kw)
        with pytest.raises(GeosradError, match=what) as e:
            dev_icarus(ctx, small, m, a["th"], a["thd"], overlap=a["overlap"])
        assert e.value.rc == 1
    one = {k: (v[:1] if v.ndim == 2 else v) for k, v in b.items()}
    one["phalf"] = b["phalf"][:2]
    with pytest.raises(GeosradError, match="nlev") as e:
        dev_icarus(ctx, one, fx["mask_ov3"][:1], 1, 2)
    assert e.value.rc == 1
    with pytest.raises(GeosradError, match="ncol"):
        dev_icarus(ctx, small, m[:, :0], 1, 2)
    for overlap in (0, 4):
        with pytest.raises(GeosradError, match="overlap"):
            dev_scops(ctx, b["seed"], small["cc"], small["conv"], overlap, 3)
    with pytest.raises(GeosradError, match="nlev"):
        dev_scops(ctx, b["seed"], one["cc"], one["conv"], 3, 3)
    with pytest.raises(GeosradError, match="ncol"):
        dev_scops(ctx, b["seed"], small["cc"], small["conv"], 3, 0)
    with pytest.raises(GeosradError, match="ncol"):          # the histogram counts a point's sub-columns in 16 bits
        ctx.scops_dev(_stream(), 4, 5, 65536, {}, 3)


# ---- the COSP wrapper ------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("rk,kind,dt", KINDS)
def test_cosp_seeds(gpu_ctx, rk, kind, dt):
    import torch
    ctx = gpu_ctx[rk]
    rng = np.random.default_rng(5)
    for n in (1, 2, 70, 3000):
        psfc = rng.uniform(52000.0, 104000.0, n).astype(np.float32).astype(dt)
        t = {"psfc": _dev(psfc, dt), "seed": torch.full((n,), -3, dtype=torch.int32, device="cuda")}
        ctx.cosp_seeds_dev(_stream(), n, {k: v.data_ptr() for k, v in t.items()})
        ctx.check(_stream())
        np.testing.assert_array_equal(t["seed"].cpu().numpy(), U.cosp_seeds(psfc, dt), err_msg=str(n))


@pytest.mark.gpu
@pytest.mark.parametrize("rk,kind,dt", KINDS)
@pytest.mark.parametrize("opts", [(3, 1, 2, True), (3, 3, 1, True), (2, 2, 1, False), (1, 1, 1, False)])
def test_isccp_dev_equals_the_solver_level_calls(gpu_ctx, fx, rk, kind, dt, opts):
    """geosrad_isccp_dev on model-ordered GEOS fields against the solver-level calls as COSP makes them: geosrad_scops_dev on FCLD / CCA as
    they are (cosp.F90:392-397), geosrad_icarus_dev on the arrays numpy prepares as cosp_isccp_simulator.F90:58-72 does (cc / conv times
    0.999999, which icarus reads in its range check only), and the wrapper's own two output steps in numpy: bit for bit, SGFCLD and the
    seeds included.  With and without the convective twins (NULL = zero).  Under maximum overlap without convection a sub-column's
    threshold stays (ibox - .5) / ncol, so a fraction one ulp above it is cloud in that sub-column as it is and clear times 0.999999: such
    cells are planted, and the mask must be the one of the unscaled fraction."""
    import torch
    overlap, th, thd, conv = opts
    ctx = gpu_ctx[rk]
    f = U.model_fields(_batch(fx))
    if not conv:
        f["CCA"] = f["DTAU_C"] = f["DEM_C"] = None
    planted = overlap == 1 and not conv
    if planted:
        f["FCLD"] = f["FCLD"].astype(dt)
        for ibox in (3, 11, 30):
            f["FCLD"][40 + ibox % 7, 2 * ibox] = np.nextafter((dt(ibox) - dt(.5)) / dt(NCOL), dt(1))
        f["FCLD"][50, 7] = 1.0000005 if dt is np.float32 else 1.0 + 5e-7      # in range only as icarus sees it, times 0.999999
    lm, npts = f["T"].shape
    names = ["T", "QV", "FCLD", "CCA", "PLE", "PLO", "DTAU_S", "EMISS", "DTAU_C", "DEM_C", "TS"]
    t = {k: _dev(f[k], dt) for k in names if f[k] is not None}
    t["sunlit"] = _dev(f["sunlit"], np.int32); t["seed"] = _dev(f["seed"], np.int32)
    o = _out_tensors(t["TS"].dtype, npts, NCOL)
    o["SGFCLD"] = torch.full((lm, npts), CANARY, dtype=t["TS"].dtype, device="cuda")
    ptr = {k: v.data_ptr() for k, v in {**t, **o}.items()}
    ws0 = ctx.workspace_bytes()
    ctx.isccp_dev(_stream(), npts, lm, NCOL, ptr, overlap=overlap, top_height=th, top_height_direction=thd, emsfc_lw=U.EMSFC_LW)
    ctx.check(_stream())
    torch.cuda.synchronize()
    assert ctx.workspace_bytes() >= max(ws0, npts * NCOL * lm)      # the mask is the context's
    got = {k: v.cpu().numpy() for k, v in o.items()}
    p = U.cosp_prepare(f, dt)
    p["sunlit"] = f["sunlit"]
    fcld, cca = np.asarray(f["FCLD"], dt), np.zeros_like(p["cc"]) if f["CCA"] is None else np.asarray(f["CCA"], dt)
    mask, seed = dev_scops(ctx, f["seed"], fcld, cca, overlap, NCOL)
    np.testing.assert_array_equal(t["seed"].cpu().numpy(), seed)
    want = U.cosp_finish(dev_icarus(ctx, p, mask, th, thd, overlap=overlap), dt)
    for n in U.ICARUS_OUT:
        np.testing.assert_array_equal(got[n], want[n], err_msg=n)
    np.testing.assert_array_equal(got["SGFCLD"], U.sgfcld(mask, dt))
    assert (not conv or (mask == 2).any()) and (got["SGFCLD"] > 0).sum() > 200
    rm, rs = U.scops(f["seed"], fcld, cca, overlap, NCOL, dt)      # the fields themselves, not the scaled fractions, went into SCOPS
    np.testing.assert_array_equal(mask, rm); np.testing.assert_array_equal(seed, rs)
    if planted:
        sm, _ = U.scops(f["seed"], p["cc"], p["conv"], overlap, NCOL, dt)
        for ibox in (3, 11, 30):
            assert mask[40 + ibox % 7, ibox - 1, 2 * ibox] == 1 and sm[40 + ibox % 7, ibox - 1, 2 * ibox] == 0
        assert got["SGFCLD"][50, 7] == 1 and not np.array_equal(got["SGFCLD"], U.sgfcld(sm, dt))


# ---- host variants ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("rk,kind,dt", KINDS)
@pytest.mark.parametrize("copies,chunk", [(2, 64), (1, 64)])
def test_host_variants_equal_the_device_ones_across_chunks(gpu_ctx, fx, rk, kind, dt, copies, chunk):
    ctx = gpu_ctx[rk]
    b = {k: np.ascontiguousarray(np.concatenate([v] * copies, axis=-1)) for k, v in _batch(fx).items()}
    b["seed"] = (b["seed"] + np.arange(b["seed"].size, dtype=np.int32) // 96 * 13).astype(np.int32)      # the second copy: other streams
    nlev, npts = b["pfull"].shape
    dmask, dseed = dev_scops(ctx, b["seed"], b["cc"], b["conv"], 3, NCOL)
    dev = dev_icarus(ctx, b, dmask, 1, 2)
    ctx.set_chunk(chunk)
    try:
        hmask, hseed = ctx.scops(npts, nlev, NCOL, b["seed"], b["cc"], b["conv"], 3)
        host = ctx.icarus(npts, b["sunlit"], nlev, NCOL, b["pfull"], b["phalf"], b["qv"], b["cc"], b["conv"], b["dtau_s"], b["dtau_c"], 1, 2, 3, hmask,
                          b["skt"], U.EMSFC_LW, b["at"], b["dem_s"], b["dem_c"])
        some = ctx.icarus(npts, b["sunlit"], nlev, NCOL, b["pfull"], b["phalf"], b["qv"], b["cc"], b["conv"], b["dtau_s"], b["dtau_c"], 1, 2, 3, hmask,
                          b["skt"], U.EMSFC_LW, b["at"], b["dem_s"], b["dem_c"], want=("boxptop", "meantb"))
    finally:
        ctx.set_chunk(131072)
    assert hmask.dtype == dt and hmask.shape == (nlev, NCOL, npts)
    np.testing.assert_array_equal(hmask, dmask.astype(dt))
    np.testing.assert_array_equal(hseed, dseed)
    if copies == 1:
        np.testing.assert_array_equal(dmask, fx["mask_ov3"])
    for n in U.ICARUS_OUT:
        np.testing.assert_array_equal(host[n], dev[n], err_msg=n)
    assert set(some) == {"boxptop", "meantb"}
    np.testing.assert_array_equal(some["boxptop"], dev["boxptop"]); np.testing.assert_array_equal(some["meantb"], dev["meantb"])
