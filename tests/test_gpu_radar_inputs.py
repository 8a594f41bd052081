"""GPU (pytest -m gpu): the radar simulator's front end of include/geosrad_radar.h - geosrad_prec_scops[_dev], geosrad_cosp_sghydro[_dev],
geosrad_radar_gases[_dev] - against what the reference's own Fortran wrote into tests/golden/satsim_radar_inputs_72.npz, and at the shapes
the fixture does not hold against the numpy restatements that tests/test_radar_inputs_oracle.py pins to it.

Bounds (the issue's).  prec_frac: the reference's bytes, in every cell, in both kinds.  The sub-grid contents: bitwise the restatement's in
both kinds (counts and IEEE divisions).  g_vol and g_to_vol against the reference: 8 x the fixture's restate64rel_* of that output, the
largest relative difference of the float64 numpy restatement from the reference - two correct double evaluations that differ in libm land in
that range, and 8 x allows for the device library's pow / exp being a couple of ulp looser than glibc's.  Where the comparison is with the
restatement itself (the small nlev) the bound is 9 x: the restatement lies within 1 x of the reference.  Every comparison prints its measured
figure (pytest -s); profiles/satsim_radar_inputs.md keeps them."""
import numpy as np
import pytest

from tests import radar_inputs_util as RU

KINDS = [(4, "r4", np.float32), (8, "r8", np.float64)]
CANARY = -7.0
SG_REAL = ["frac_ls", "frac_cv", "prec_ls", "prec_cv", "mr_sub", "mr_hydro_sg"]
MR = ["mr_" + c for c in RU.CLASSES]


@pytest.fixture(scope="module")
def b():
    return RU.load_batch()


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def _dev(a, dt):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).cuda()


def dev_prec_scops(ctx, ls, cv, mask):
    import torch
    nlev, ncol, npts = mask.shape
    t = dict(ls_p_rate=_dev(ls, ctx.dtype), cv_p_rate=_dev(cv, ctx.dtype), frac_out_u8=_dev(mask, np.uint8))
    out = torch.full(mask.shape, 77, dtype=torch.uint8, device="cuda")
    ptr = {k: v.data_ptr() for k, v in t.items()}
    ptr["prec_frac_u8"] = out.data_ptr()
    try:
        ctx.prec_scops_dev(_stream(), npts, nlev, ncol, ptr)
        ctx.check(_stream())
    finally:
        torch.cuda.synchronize()
    return out.cpu().numpy()


def dev_sghydro(ctx, mask, mr, want=("prec_frac_u8",) + tuple(SG_REAL)):
    """geosrad_cosp_sghydro_dev on device copies; a class that is None is passed as NULL; every output is allocated and canary-filled, those in
    `want` are passed"""
    import torch
    nlev, ncol, npts = mask.shape
    t = {n: _dev(a, ctx.dtype) for n, a in zip(MR, mr) if a is not None}
    t["frac_out_u8"] = _dev(mask, np.uint8)
    tdt = torch.float32 if ctx.dtype == np.float32 else torch.float64
    shapes = {"mr_sub": (9, nlev, npts), "mr_hydro_sg": (9, nlev, ncol, npts)}
    o = {k: torch.full(shapes.get(k, (nlev, npts)), CANARY, dtype=tdt, device="cuda") for k in SG_REAL}
    o["prec_frac_u8"] = torch.full(mask.shape, 77, dtype=torch.uint8, device="cuda")
    ptr = {k: v.data_ptr() for k, v in t.items()}
    ptr.update({k: o[k].data_ptr() for k in want})
    try:
        ctx.cosp_sghydro_dev(_stream(), npts, nlev, ncol, ptr)
        ctx.check(_stream())
    finally:
        torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in o.items()}


def dev_gases(ctx, p, t, rh, zlev, freq, sr, want=("g_vol", "g_to_vol"), check=True):
    import torch
    nlev, npts = np.shape(p)
    d = dict(p=_dev(p, ctx.dtype), t=_dev(t, ctx.dtype), rh=_dev(rh, ctx.dtype), zlev=_dev(zlev, ctx.dtype))
    o = {k: torch.full((nlev, npts), CANARY, dtype=torch.float64, device="cuda") for k in ("g_vol", "g_to_vol")}
    ptr = {k: v.data_ptr() for k, v in d.items()}
    ptr.update({k: o[k].data_ptr() for k in want})
    try:
        ctx.radar_gases_dev(_stream(), npts, nlev, ptr, freq, sr)
        if check:
            ctx.check(_stream())
    finally:
        torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in o.items()}


def _relmax(got, ref):
    return float((np.abs(got - ref) / np.maximum(np.abs(ref), 1e-300)).max())


# ---- prec_scops ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("rk,kind,dt", KINDS)
def test_prec_frac_equals_the_reference(gpu_ctx, b, rk, kind, dt):
    ls, cv = RU.rates(b["mr"], dt)
    got = dev_prec_scops(gpu_ctx[rk], ls, cv, b["mask"])
    diff = int((got != b["fx"]["prec_frac"]).sum())
    print(f"{kind}: {diff} of {got.size} cells of prec_frac differ from the reference's")
    assert diff == 0


# every npoints of 1, 63, 65, 130, nlev of 2, 3 and ncol of 1, 19, 20, 40, 64, 65 (19 | 20 | 40: cv_col 1 | 1 | 2; 63 | 65: a wave and a lane more)
EDGE = [(1, 2, 1), (63, 3, 19), (65, 2, 20), (130, 3, 40), (63, 2, 64), (65, 3, 65), (130, 2, 19), (1, 3, 40)]


def _random_case(npts, nlev, ncol, seed):
    rng = np.random.default_rng(seed)
    u = rng.uniform(0, 1, (nlev, ncol, npts))
    dens = rng.choice([0.0, 0.05, 0.5], (nlev, 1, npts))           # many levels without any cloud, so that THREE, Four and Five occur
    mask = np.where(u < dens, 1, np.where(u < 1.5 * dens, 2, 0)).astype(np.uint8)
    rate = lambda: np.where(rng.uniform(0, 1, (nlev, npts)) < 0.6, rng.uniform(1e-6, 1e-3, (nlev, npts)), rng.choice([0.0, -1e-5], (nlev, npts)))
    return mask, rate(), rate()


@pytest.mark.gpu
@pytest.mark.parametrize("rk,kind,dt", KINDS)
def test_prec_frac_at_the_edge_shapes(gpu_ctx, rk, kind, dt):
    seen = set()
    for i, (npts, nlev, ncol) in enumerate(EDGE):
        mask, ls, cv = _random_case(npts, nlev, ncol, 100 + i)
        want, pl, pc = RU.prec_scops(ls.astype(dt), cv.astype(dt), mask, dt, detail=True)
        got = dev_prec_scops(gpu_ctx[rk], ls, cv, mask)
        assert np.array_equal(got, want), (npts, nlev, ncol, int((got != want).sum()))
        seen |= set(np.unique(pl)) | set(np.unique(pc))
    assert seen == {0, 1, 2, 3, 4, 5}


@pytest.mark.gpu
@pytest.mark.parametrize("rk,kind,dt", KINDS)
def test_each_possibility_alone(gpu_ctx, rk, kind, dt):
    """nlev = 3, ncol = 40 (cv_col = 2), one point a possibility, the same for both kinds: the second level's precipitation is placed by
    ONE (cloud in the level), TWO (precipitation above), THREE (cloud below), Four (cloud in the column: only above, in a dry level), Five"""
    nlev, ncol, npts = 3, 40, 5
    mask = np.zeros((nlev, ncol, npts), np.uint8)
    ls = np.zeros((nlev, npts)); cv = np.zeros((nlev, npts))
    ls[1] = cv[1] = 1e-4
    mask[1, 3:6, 0] = 1; mask[1, 30:32, 0] = 2                       # ONE
    mask[0, 7:9, 1] = 1; mask[0, 11, 1] = 2; ls[0, 1] = cv[0, 1] = 1e-4          # TWO: the first level's ONE, handed down
    mask[2, 20:25, 2] = 1; mask[2, 1, 2] = 2                         # THREE
    mask[0, 15, 3] = 1; mask[0, 16:18, 3] = 2                        # Four: cloud in a first level without precipitation
    want, pl, pc = RU.prec_scops(ls.astype(dt), cv.astype(dt), mask, dt, detail=True)
    assert pl[1].tolist() == pc[1].tolist() == [1, 2, 3, 4, 5]
    got = dev_prec_scops(gpu_ctx[rk], ls, cv, mask)
    assert np.array_equal(got, want)
    col = lambda j: got[1, :, j].tolist()
    z = [0] * ncol
    e0 = list(z); e0[3:6] = [1] * 3; e0[30:32] = [2] * 2
    e1 = list(z); e1[7:9] = [1] * 2; e1[11] = 2
    e2 = list(z); e2[20:25] = [1] * 5; e2[1] = 2
    e3 = list(z); e3[15] = 1; e3[16:18] = [2] * 2
    e4 = [3, 3] + [1] * (ncol - 2)
    assert [col(j) for j in range(5)] == [e0, e1, e2, e3, e4]
    assert (got[2] == 0).all() and (got[0, :, [0, 2, 3, 4]] == 0).all()


# ---- the sub-grid hydrometeor contents -----------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("rk,kind,dt", KINDS)
def test_sghydro_is_the_restatement_bit_for_bit(gpu_ctx, b, rk, kind, dt):
    mask, mr = b["mask"], b["mr"]
    got = dev_sghydro(gpu_ctx[rk], mask, mr)
    ref = RU.sghydro(mask, mr, dt)
    assert np.array_equal(got["prec_frac_u8"], b["fx"]["prec_frac"])
    for n in ("frac_ls", "frac_cv", "prec_ls", "prec_cv", "mr_sub"):
        assert got[n].dtype == dt
        np.testing.assert_array_equal(got[n], ref[n], err_msg=n)
    # the expanded output is the index rule on mr_sub: by the cloud mask, the precipitation classes too
    np.testing.assert_array_equal(got["mr_hydro_sg"], RU.expand(mask, ref["mr_sub"]))
    assert (got["mr_hydro_sg"][2][mask != 1] == 0).all() and (got["mr_hydro_sg"][2] > 0).any() and (got["mr_hydro_sg"][6] > 0).any()
    # only what is asked for is written, and it does not depend on what else is; NULL classes are zero
    part = dev_sghydro(gpu_ctx[rk], mask, mr[:4] + [None] * 5, want=("prec_ls", "mr_hydro_sg"))
    ref2 = RU.sghydro(mask, mr[:4] + [None] * 5, dt)
    np.testing.assert_array_equal(part["prec_ls"], ref2["prec_ls"])
    np.testing.assert_array_equal(part["mr_hydro_sg"], RU.expand(mask, ref2["mr_sub"]))
    for n in ("frac_ls", "frac_cv", "prec_cv", "mr_sub"):
        assert (part[n] == dt(CANARY)).all(), n
    assert (part["prec_frac_u8"] == 77).all()


@pytest.mark.gpu
@pytest.mark.parametrize("rk,kind,dt", KINDS)
def test_sghydro_at_the_edge_shapes(gpu_ctx, rk, kind, dt):
    for i, (npts, nlev, ncol) in enumerate(EDGE[:6]):
        mask, ls, cv = _random_case(npts, nlev, ncol, 200 + i)
        rng = np.random.default_rng(300 + i)
        mr = [rng.uniform(0, 1e-3, (nlev, npts)).astype(np.float32) for _ in range(9)]
        mr[2], mr[6] = np.maximum(ls, 0).astype(np.float32), np.maximum(cv, 0).astype(np.float32)
        got = dev_sghydro(gpu_ctx[rk], mask, mr)
        ref = RU.sghydro(mask, mr, dt)
        assert np.array_equal(got["prec_frac_u8"], ref["prec_frac"]), (npts, nlev, ncol)
        for n in ("frac_ls", "frac_cv", "prec_ls", "prec_cv", "mr_sub"):
            np.testing.assert_array_equal(got[n], ref[n], err_msg=f"{n} {npts} {nlev} {ncol}")
        np.testing.assert_array_equal(got["mr_hydro_sg"], RU.expand(mask, ref["mr_sub"]))


# ---- gases ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("sr", [0, 1])
@pytest.mark.parametrize("rk,kind,dt", KINDS)
def test_gases_against_the_reference(gpu_ctx, b, rk, kind, dt, sr):
    fx = b["fx"]
    got = dev_gases(gpu_ctx[rk], b["p"], b["t"], b["rh"], b["zlev"], float(fx["freq"]), sr)
    for n, ref in (("g_vol", fx[f"{kind}_g_vol"]), ("g_to_vol", fx[f"{kind}_g_to_vol_sr{sr}"])):
        bound = 8.0 * float(fx[f"restate64rel_{n}"])
        rel = _relmax(got[n], ref)
        print(f"{kind} surface_radar={sr} {n}: max rel |device - reference| = {rel:.3e} (bound {bound:.3e} = 8 x {float(fx['restate64rel_' + n]):.3e})")
        assert got[n].dtype == np.float64 and rel <= bound, (n, rel, bound)
    first = got["g_to_vol"].shape[0] - 1 if sr else 0
    assert (got["g_to_vol"][first] == 0).all()
    # g_vol alone: the path kernels are skipped and g_to_vol is untouched
    only = dev_gases(gpu_ctx[rk], b["p"], b["t"], b["rh"], b["zlev"], float(fx["freq"]), sr, want=("g_vol",))
    assert np.array_equal(only["g_vol"], got["g_vol"]) and (only["g_to_vol"] == CANARY).all()


@pytest.mark.gpu
@pytest.mark.parametrize("rk,kind,dt", KINDS)
def test_gases_across_the_three_point_branch(gpu_ctx, b, rk, kind, dt):
    """nlev 2, 4, 5: paths of 1 to 3 points only (math_lib.f90:145-150), and one gate of AVINT on 4 points; npoints 65: a lane past a wave"""
    fx = b["fx"]
    for nlev in (2, 4, 5):
        for sr in (0, 1):
            sl = (slice(40, 40 + nlev), slice(0, 65))
            p, t, rh, z = (np.ascontiguousarray(b[k][sl]) for k in ("p", "t", "rh", "zlev"))
            got = dev_gases(gpu_ctx[rk], p, t, rh, z, float(fx["freq"]), sr)
            ref = RU.radar_gases(p, t, rh, z, float(fx["freq"]), sr, dt)
            for n, r in zip(("g_vol", "g_to_vol"), ref):
                bound = 9.0 * float(fx[f"restate64rel_{n}"])
                rel = _relmax(got[n], r)
                print(f"{kind} nlev={nlev} surface_radar={sr} {n}: max rel |device - restatement| = {rel:.3e} (bound {bound:.3e})")
                assert rel <= bound, (nlev, sr, n, rel)


# ---- host variants, chunks and shards ----------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("rk,kind,dt", KINDS)
def test_host_variants_equal_the_device_ones_across_chunks_and_shards(gpu_ctx, b, rk, kind, dt):
    from geosradiation_gridcomp_amd.api import Context
    ctx = gpu_ctx[rk]
    two = lambda a: np.ascontiguousarray(np.concatenate([a, a[..., ::-1][..., :37]], axis=-1))          # 133 points: ragged at a chunk of 64
    mask, mr = two(b["mask"]), [two(m) for m in b["mr"]]
    p, t, rh, z = (two(b[k]) for k in ("p", "t", "rh", "zlev"))
    ls, cv = RU.rates(mr, dt)
    nlev, ncol, npts = mask.shape
    freq = float(b["fx"]["freq"])
    dev_pf = dev_prec_scops(ctx, ls, cv, mask)
    dev_sg = dev_sghydro(ctx, mask, mr)
    dev_g = dev_gases(ctx, p, t, rh, z, freq, 0)
    want = ("prec_frac",) + tuple(SG_REAL)

    def host(c):
        return (c.prec_scops(npts, nlev, ncol, ls, cv, mask.astype(dt)), c.cosp_sghydro(npts, nlev, ncol, mask.astype(dt), *mr, want=want),
                c.radar_gases(npts, nlev, p, t, rh, z, freq, 0))
    ctx.set_chunk(64)
    try:
        runs = {"chunked": host(ctx)}
    finally:
        ctx.set_chunk(131072)
    multi = Context(rk, devices=[0, 0], tables=False)
    try:
        runs["sharded"] = host(multi)
    finally:
        multi.close()
    for tag, (pf, sg, g) in runs.items():
        assert pf.dtype == dt and np.array_equal(pf, dev_pf.astype(dt)), tag
        assert np.array_equal(sg["prec_frac"], dev_pf.astype(dt)), tag
        for n in SG_REAL:
            np.testing.assert_array_equal(sg[n], dev_sg[n], err_msg=f"{tag} {n}")
        for n in ("g_vol", "g_to_vol"):
            assert g[n].dtype == np.float64
            np.testing.assert_array_equal(g[n], dev_g[n], err_msg=f"{tag} {n}")
    assert np.array_equal(dev_pf[..., :96], b["fx"]["prec_frac"])


# ---- refusals ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("rk,kind,dt", KINDS)
def test_refusals(gpu_ctx, b, rk, kind, dt):
    from geosradiation_gridcomp_amd.api import GeosradError, GeosradInputError
    ctx = gpu_ctx[rk]
    sl = (slice(50, 56), slice(0, 70))
    p, t, rh, z = (np.ascontiguousarray(b[k][sl], dtype=dt) for k in ("p", "t", "rh", "zlev"))
    nlev, npts = p.shape
    ncol = 4
    mask = np.zeros((nlev, ncol, npts), dt)
    mr = [np.zeros((nlev, npts), dt)] * 9

    def einval(fn, match):
        with pytest.raises(GeosradError, match=match) as e:
            fn()
        assert e.value.rc == 1 and not isinstance(e.value, GeosradInputError)
    # GEOSRAD_EINVAL, before anything runs
    for bad_np, bad_nlev, bad_ncol, match in ((0, nlev, ncol, "npoints"), (npts, 1, ncol, "nlev"), (npts, nlev, 0, "ncol"), (npts, nlev, 65536, "ncol")):
        einval(lambda: ctx.prec_scops(bad_np, bad_nlev, bad_ncol, p, p, mask), "geosrad_prec_scops: " + match)
        einval(lambda: ctx.cosp_sghydro(bad_np, bad_nlev, bad_ncol, mask, *mr), "geosrad_cosp_sghydro: " + match)
    einval(lambda: ctx.radar_gases(0, nlev, p, t, rh, z, 94.0), "geosrad_radar_gases: npoints")
    einval(lambda: ctx.radar_gases(npts, 1, p, t, rh, z, 94.0), "geosrad_radar_gases: nlev")
    einval(lambda: ctx.radar_gases(npts, nlev, p, t, rh, z, 94.0, surface_radar=2), "surface_radar must be 0 or 1")
    einval(lambda: ctx.radar_gases(npts, nlev, p, t, rh, z, 94.0, surface_radar=-1), "surface_radar must be 0 or 1")
    einval(lambda: ctx.radar_gases(npts, nlev, p, t, rh, z, 0.0), "freq must be positive")
    einval(lambda: ctx.radar_gases(npts, nlev, p, t, rh, z, -94.0), "freq must be positive")
    einval(lambda: ctx.radar_gases(npts, nlev, p, None, rh, z, 94.0), "null input array")
    einval(lambda: ctx.prec_scops(npts, nlev, ncol, p, None, mask), "null array")
    einval(lambda: ctx.cosp_sghydro(npts, nlev, ncol, mask, mr[0], mr[1], None, mr[3]), "null input array")
    einval(lambda: ctx.cosp_sghydro(npts, nlev, ncol, None, *mr), "null input array")
    einval(lambda: ctx.radar_gases_dev(_stream(), npts, nlev, {}, 94.0), "null input array")
    # GEOSRAD_EINPUT through the device error word, with the array's name: the `_dev` variant from geosrad_check, the host variant itself
    def flip(a, v):
        c = a.copy(); c[3, 66] = v
        return c
    zbad = z.copy(); zbad[2, 65] = zbad[3, 65]                     # two equal heights: not strictly decreasing
    zup = np.ascontiguousarray(z[::-1])                            # ascending: the order a surface radar's gates have, not its input's
    for args, name in (((flip(p, 0.0), t, rh, z), "p"), ((flip(p, -5.0), t, rh, z), "p"), ((p, flip(t, 0.0), rh, z), "t"), ((p, t, rh, zbad), "zlev"),
                       ((p, t, rh, zup), "zlev")):
        assert RU.gases_range_check(*args[:2], args[3]) == name
        for sr in (0, 1):
            dev_gases(ctx, *args, 94.0, sr, check=False)
            with pytest.raises(GeosradInputError, match=rf"radar_gases\): {name}") as e:
                ctx.check(_stream())
            assert e.value.rc == 5
            ctx.check(_stream())                    # reported once; the flag is down again
            with pytest.raises(GeosradInputError, match=rf"radar_gases\): {name}") as e:
                ctx.radar_gases(npts, nlev, *args, 94.0, sr)
            assert e.value.rc == 5
            ctx.check(_stream())
    good = dev_gases(ctx, p, t, rh, z, 94.0, 0)
    assert np.isfinite(good["g_vol"]).all() and (good["g_vol"] > 0).all()
