"""GPU (pytest -m gpu): the MISR simulator of include/geosrad_misr_modis.h - geosrad_misr_dev and geosrad_misr - in an fp32 context against
what the reference's r4 build wrote into tests/golden/satsim_misr_modis_72.npz and in an fp64 context against its r8 build, for the batch
as it is and rolled by one point; for the shapes the fixture does not hold against the numpy restatement that
tests/test_satsim_misr_modis_oracle.py pins to the same fixture.

Bounds against the fixture (the issue's).  Histogram: fp64 no sub-column in another cell; fp32 at most 0.2 % of the batch's cloudy
sub-columns (the cap of tests/test_gpu_satsim.py; the reference's own two builds move none).  dist_model_layertops and every
missing_value position: identical.  MISR_mean_ztop, MISR_cldarea: fp32 against r4 within 4 x the fixture's own r4-r8 spread of that output
or, where that is larger, 4 fp32 ulps of the output's largest magnitude; fp64 against r8 within 64 eps relative (restate64_* is 0).  Every
comparison prints its measured figure (pytest -s); DESIGN.md 4.13 keeps them.

Against the restatement the comparison is an equality: MISR_simulator.f has no transcendental but the constant tauchk = -log(0.9999999),
every other operation is an IEEE add, multiply or divide that the kernels do in the reference's order with contraction off, and the
restatement equals both builds of the reference bit for bit."""
import numpy as np
import pytest

from tests import satsim_util as U
from tests import satsim_misr_modis_util as M

KINDS = [(4, "r4", np.float32), (8, "r8", np.float64)]
CANARY = -7.0
NCOL = 30
IN = ["zfull", "at", "dtau_s", "dtau_c"]


@pytest.fixture(scope="module")
def fx():
    f, g = np.load(M.FIXTURE), np.load(U.FIXTURE)
    d = {k: f[k] for k in f.files}
    d.update({k: g[k] for k in g.files if k.startswith("in_") or k == "mask_ov3"})
    return d


def _batch(fx, rolled=False):
    b = {k: fx["in_" + k] for k in ["sunlit"] + IN}
    b["mask"] = fx["mask_ov3"]
    return {k: M.roll1(v) for k, v in b.items()} if rolled else b


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def _dev(a, dt):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).cuda()


def dev_misr(ctx, b, want=M.MISR_OUT, missing=M.MISSING, drop=()):
    """geosrad_misr_dev on device copies of the batch; every output is allocated and canary-filled, those in `want` are passed; the
    inputs named in `drop` are passed as NULL"""
    import torch
    nlev, ncol, npts = b["mask"].shape
    t = {k: _dev(b[k], ctx.dtype) for k in IN}
    t["sunlit"] = _dev(b["sunlit"], np.int32)
    t["frac_out_u8"] = _dev(b["mask"], np.uint8)
    shapes = {"fq_MISR_TAU_v_CTH": (16, 7, npts), "dist_model_layertops": (16, npts)}
    o = {k: torch.full(shapes.get(k, (npts,)), CANARY, dtype=t["at"].dtype, device="cuda") for k in M.MISR_OUT}
    ptr = {k: v.data_ptr() for k, v in t.items() if k not in drop}
    ptr.update({k: o[k].data_ptr() for k in want})
    try:
        ctx.misr_dev(_stream(), npts, nlev, ncol, ptr, missing)
        ctx.check(_stream())
    finally:
        torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in o.items()}


def restate(b, dt, missing=M.MISSING):
    return M.misr(b["sunlit"], b["zfull"], b["at"], b["dtau_s"], b["dtau_c"], b["mask"], missing, dt)


def check_misr(got, fx, kind, dt, tag, label):
    eps = float(np.finfo(dt).eps)
    miss = dt(M.MISSING)
    ref = {n: fx[f"{kind}_{n}{tag}"] for n in M.MISR_OUT}
    for n in M.MISR_OUT:
        assert got[n].dtype == ref[n].dtype == dt and got[n].shape == ref[n].shape, (label, n)
        assert np.array_equal(got[n] == miss, ref[n] == miss), (label, n, "missing values")
    gc, rc = M.misr_counts(got["fq_MISR_TAU_v_CTH"], NCOL), M.misr_counts(ref["fq_MISR_TAU_v_CTH"], NCOL)
    cloudy = int(rc.sum())
    moved = int(np.abs(gc - rc).sum() + 1) // 2
    print(f"{label}: {moved} of {cloudy} histogram sub-columns in another cell")
    assert moved <= (0.002 * cloudy if dt is np.float32 else 0), (label, moved, cloudy)
    if moved == 0:
        np.testing.assert_array_equal(got["fq_MISR_TAU_v_CTH"], ref["fq_MISR_TAU_v_CTH"], err_msg=label)
    np.testing.assert_array_equal(got["dist_model_layertops"], ref["dist_model_layertops"], err_msg=label)
    for n in M.MISR_CONTINUOUS:
        ok = ref[n] != miss
        g, r = got[n].astype(np.float64)[ok], ref[n].astype(np.float64)[ok]
        d = np.abs(g - r)
        if dt is np.float32:
            spread, floor = float(fx[f"spread_{n}{tag}"]), 4 * float(np.finfo(np.float32).eps) * float(np.abs(r).max())
            bound = max(4 * spread, floor)
            print(f"{label} {n}: max |dev - ref| = {d.max():.3e} = {d.max() / max(spread, 1e-300):.2f} x the reference's r4-r8 spread {spread:.2e} "
                  f"(bound {bound:.2e})")
            assert d.max() <= bound, (label, n, float(d.max()), bound)
        else:
            rel = max(64 * eps, 0.0)
            assert 4 * float(fx[f"restate64_{n}{tag}"]) == 0.0
            e = d / np.maximum(np.abs(r), 1e-300)
            e[d == 0] = 0
            print(f"{label} {n}: max rel = {e.max():.3e} = {e.max() / eps:.1f} eps (bound 64 eps)")
            assert (d <= rel * np.abs(r)).all(), (label, n, float(e.max()))


@pytest.fixture(scope="module")
def misr_runs(gpu_ctx, fx):
    """every (kind, order) once, all outputs, shared by the tests below"""
    return {(rk, rolled): dev_misr(gpu_ctx[rk], _batch(fx, rolled)) for rk, _, _ in KINDS for rolled in (False, True)}


@pytest.mark.gpu
@pytest.mark.parametrize("rk,kind,dt", KINDS)
def test_misr_against_the_reference(misr_runs, fx, rk, kind, dt):
    got = misr_runs[(rk, False)]
    check_misr(got, fx, kind, dt, "", f"{kind} MISR")
    miss = dt(M.MISSING)
    dark = fx["in_sunlit"] != 1
    # the dark-point rules: missing in three outputs, MISR_mean_ztop 0 except for the call's last point
    assert (got["fq_MISR_TAU_v_CTH"][:, :, dark] == miss).all() and (got["dist_model_layertops"][:, dark] == miss).all()
    assert (got["MISR_cldarea"][dark] == miss).all() and (got["MISR_mean_ztop"][dark][:-1] == 0).all() and got["MISR_mean_ztop"][-1] == miss
    cnt = M.misr_counts(got["fq_MISR_TAU_v_CTH"], NCOL)
    assert cnt[0].sum() == 124 and (got["MISR_cldarea"][~dark] > 0).sum() == 56


@pytest.mark.gpu
@pytest.mark.parametrize("rk,kind,dt", KINDS)
def test_rolled_batch_point_1_first(misr_runs, fx, rk, kind, dt):
    """the pattern matcher works on the call's first point only: the batch's point 1 is 300 m higher when it is first; the batch's sunlit
    point 0, now last, keeps its own MISR_mean_ztop"""
    got, asis = misr_runs[(rk, True)], misr_runs[(rk, False)]
    check_misr(got, fx, kind, dt, "_rolled", f"{kind} MISR rolled")
    assert abs(float(got["MISR_mean_ztop"][0]) - 5979.99) < 0.02 and abs(float(asis["MISR_mean_ztop"][1]) - 5680.75) < 0.02
    np.testing.assert_array_equal(got["MISR_mean_ztop"][1:-2], asis["MISR_mean_ztop"][2:-1])          # every other point is untouched
    assert got["MISR_mean_ztop"][-2] == 0 and got["MISR_mean_ztop"][-1] != dt(M.MISSING)


@pytest.mark.gpu
@pytest.mark.parametrize("rk,kind,dt", KINDS)
@pytest.mark.parametrize("npts,ncol,nlev", [(70, 30, 24), (96, 2, 24), (96, 7, 24), (300, 30, 3), (70, 7, 2)])
def test_other_shapes_equal_the_restatement(gpu_ctx, rk, kind, dt, npts, ncol, nlev):
    """a partial wavefront of points, two and seven sub-columns, three and two levels (every level the first or the last), more than one
    block of points; the last point dark (300 points) or sunlit (70 and 96 after the roll)"""
    b = U.make_batch(npts, nlev, seed=91 + npts + ncol)
    b.update(M.make_hydro(b, seed=5 + nlev))
    if nlev <= 3:      # make_batch's decks need a quarter of many levels: thick cloud in two points out of three instead
        rng = np.random.default_rng(nlev)
        on = (np.arange(npts) % 3 != 0)[None, :] & (rng.uniform(0, 1, (nlev, npts)) < 0.7)
        b["cc"] = np.where(on, rng.uniform(0.2, 1.0, (nlev, npts)), 0).astype(np.float32)
        b["dtau_s"] = np.where(on, 0.05 * np.exp(5.0 * rng.uniform(0, 1, (nlev, npts))), 0).astype(np.float32)
        b["conv"] = np.zeros_like(b["cc"])
    b["mask"], _ = U.scops(b["seed"], b["cc"], b["conv"], 3, ncol, np.float32)
    if npts != 300:
        b = {k: M.roll1(v) for k, v in b.items()}
    want = restate(b, dt)
    got = dev_misr(gpu_ctx[rk], b)
    for n in M.MISR_OUT:
        np.testing.assert_array_equal(got[n], want[n], err_msg=n)
    lit = b["sunlit"] == 1
    assert (want["MISR_cldarea"][lit] > 0).sum() > npts // 4 and (b["sunlit"][-1] == 1) == (npts != 300)


@pytest.mark.gpu
@pytest.mark.parametrize("rk,kind,dt", KINDS)
def test_missing_value_and_null_outputs(gpu_ctx, misr_runs, fx, rk, kind, dt):
    """a positive missing_value goes through the reference's `if (MISR_cldarea(j) .gt. 0.)` division: 0 for a dark point, 1 for a dark last
    one; an output passed as NULL is not written and changes no other output's bits"""
    b = _batch(fx)
    got = dev_misr(gpu_ctx[rk], b, missing=9999.0)
    want = restate(b, dt, 9999.0)
    for n in M.MISR_OUT:
        np.testing.assert_array_equal(got[n], want[n], err_msg=n)
    dark = b["sunlit"] != 1
    assert (got["MISR_mean_ztop"][dark][:-1] == 0).all() and got["MISR_mean_ztop"][-1] == 1 and (got["MISR_cldarea"][dark] == 9999).all()
    full = misr_runs[(rk, False)]
    for drop in (("fq_MISR_TAU_v_CTH",), ("dist_model_layertops", "MISR_cldarea"), ("MISR_mean_ztop",)):
        got = dev_misr(gpu_ctx[rk], b, want=[n for n in M.MISR_OUT if n not in drop])
        for n in M.MISR_OUT:
            if n in drop:
                assert (got[n] == dt(CANARY)).all(), n
            else:
                np.testing.assert_array_equal(got[n], full[n], err_msg=f"{n} without {drop}")


@pytest.mark.gpu
def test_refusals(gpu_ctx, fx):
    from geosradiation_gridcomp_amd.api import GeosradError
    ctx = gpu_ctx[4]
    b = _batch(fx)
    small = {k: (v[:4] if v.ndim >= 2 else v) for k, v in b.items()}
    with pytest.raises(GeosradError, match="ncol") as e:          # the reference's serial scan over the points
        dev_misr(ctx, dict(small, mask=small["mask"][:, :1]))
    assert e.value.rc == 1
    with pytest.raises(GeosradError, match="nlev") as e:
        dev_misr(ctx, {k: (v[:1] if v.ndim >= 2 else v) for k, v in b.items()})
    assert e.value.rc == 1
    for name in ("zfull", "dtau_c", "sunlit", "frac_out_u8"):
        with pytest.raises(GeosradError, match="null") as e:
            dev_misr(ctx, small, drop=(name,))
        assert e.value.rc == 1
    with pytest.raises(GeosradError, match="ncol"):
        ctx.misr_dev(_stream(), 4, 5, 65536, {}, M.MISSING)
    with pytest.raises(GeosradError, match="npoints"):
        ctx.misr_dev(_stream(), 0, 5, 3, {}, M.MISSING)
    dev_misr(ctx, small)          # and a good call after them passes


@pytest.mark.gpu
@pytest.mark.parametrize("rk,kind,dt", KINDS)
def test_host_variant_keeps_first_and_last_across_chunks(gpu_ctx, fx, rk, kind, dt):
    """192 points in chunks of 64 (geosrad_set_chunk refuses fewer): the batch twice, turned so that its point 1 - which the pattern matcher
    lifts by 300 m when it is first - opens the second chunk, with dark points closing every chunk.  "First" and "last" are the call's:
    the second chunk's first point is not adjusted, a chunk's dark last point keeps 0 and only the call's dark last point is missing."""
    ctx = gpu_ctx[rk]
    b = {k: np.ascontiguousarray(np.roll(np.concatenate([v, v], axis=-1), 63, axis=-1)) for k, v in _batch(fx).items()}
    b["sunlit"][[63, 127, 191]] = 0
    nlev, ncol, npts = b["mask"].shape
    want = restate(b, dt)
    alone = restate({k: v[..., 64:128] for k, v in b.items()}, dt)          # what a chunk run as a call of its own would give
    assert alone["MISR_mean_ztop"][0] != want["MISR_mean_ztop"][64] and alone["MISR_mean_ztop"][-1] == dt(M.MISSING)
    dev = dev_misr(ctx, b)
    ctx.set_chunk(64)
    try:
        host = ctx.misr(npts, nlev, ncol, b["sunlit"], b["zfull"], b["at"], b["dtau_s"], b["dtau_c"], b["mask"].astype(dt), M.MISSING)
        some = ctx.misr(npts, nlev, ncol, b["sunlit"], b["zfull"], b["at"], b["dtau_s"], b["dtau_c"], b["mask"].astype(dt), M.MISSING,
                        want=("MISR_mean_ztop",))
    finally:
        ctx.set_chunk(131072)
    for n in M.MISR_OUT:
        np.testing.assert_array_equal(host[n], dev[n], err_msg=n)
        np.testing.assert_array_equal(dev[n], want[n], err_msg=n)
    assert set(some) == {"MISR_mean_ztop"}
    np.testing.assert_array_equal(some["MISR_mean_ztop"], dev["MISR_mean_ztop"])
    z = host["MISR_mean_ztop"]
    assert z[63] == 0 and z[127] == 0 and z[191] == dt(M.MISSING) and abs(float(z[64]) - 5680.75) < 0.02


@pytest.mark.gpu
@pytest.mark.parametrize("rk,kind,dt", KINDS)
def test_host_variant_keeps_first_and_last_across_shards(gpu_ctx, fx, rk, kind, dt):
    """the same 192 points through a geosrad_create_multi context of two shards of 96 on the one GPU, turned so that point 1 opens the
    second shard and a dark point closes the first: a shard is not a call - the second shard's first point is not adjusted, the first
    shard's dark last point keeps 0 and the call's dark last point is missing"""
    from geosradiation_gridcomp_amd.api import Context
    b = {k: np.ascontiguousarray(np.roll(np.concatenate([v, v], axis=-1), 95, axis=-1)) for k, v in _batch(fx).items()}
    b["sunlit"][[95, 191]] = 0
    nlev, ncol, npts = b["mask"].shape
    want = restate(b, dt)
    # a two-shard context splits 192 points as 96 + 96 (contiguous, equal shards): the two restatements below are of those very shards
    alone = restate({k: v[..., 96:] for k, v in b.items()}, dt)          # what the second shard run as a call of its own would give
    first = restate({k: v[..., :96] for k, v in b.items()}, dt)          # and the first
    assert alone["MISR_mean_ztop"][0] != want["MISR_mean_ztop"][96] and first["MISR_mean_ztop"][-1] == dt(M.MISSING) != want["MISR_mean_ztop"][95]
    dev = dev_misr(gpu_ctx[rk], b)
    multi = Context(rk, devices=[0, 0], tables=False)
    try:
        host = multi.misr(npts, nlev, ncol, b["sunlit"], b["zfull"], b["at"], b["dtau_s"], b["dtau_c"], b["mask"].astype(dt), M.MISSING)
    finally:
        multi.close()
    for n in M.MISR_OUT:
        np.testing.assert_array_equal(host[n], dev[n], err_msg=n)
        np.testing.assert_array_equal(dev[n], want[n], err_msg=n)
    z = host["MISR_mean_ztop"]
    assert z[95] == 0 and z[191] == dt(M.MISSING) and abs(float(z[96]) - 5680.75) < 0.02
