"""GPU (pytest -m gpu): the lidar simulator and the COSP path with it of include/geosrad_lidar.h - geosrad_lidar_dev, geosrad_lidar and
geosrad_cosp_lidar_dev - in an fp32 context against what the reference's r4 build (lidar_simulator per sub-column, diag_lidar) wrote into
tests/golden/satsim_lidar_72.npz and in an fp64 context against its r8 build, for ice_type 0 and 1; the shapes the fixture does not hold
against the numpy restatement that tests/test_lidar_oracle.py pins to it.

Bounds against the fixture (the issue's).  Discrete outputs - the CFAD bin of every cell, hence the cloudy / usable decisions behind lidarcld
and cldlayer, the cfad_sr counts and the undefined cells: fp64 identical to r8 in every cell; fp32 different from r4 in at most 0.2 % of the
cells, the cap tests/test_gpu_modis.py uses (the reference's own two builds differ in none of 207 360).  Continuous outputs, that test's two
rules: fp32 against r4 within 4 x the fixture's own r4-r8 spread of that output or, where that is larger, 4 fp32 ulps of the output's
largest magnitude; fp64 against r8 within the larger of 64 eps relative and 4 x what the float64 restatement differs from the r8 build
(restate64rel_*: 1 - exp(-2 tau) of a thin layer loses the digits tau is short of 1).  A (point, level) or point whose decisions differ is
left out of the comparison of lidarcld / cldlayer and counted against the cap.  Every comparison prints its measured figure (pytest -s);
DESIGN.md 4.15 keeps them."""
import numpy as np
import pytest

from tests import satsim_util as U
from tests import satsim_misr_modis_util as M
from tests import lidar_util as LU
from tests.test_lidar_oracle import batch, restate

KINDS = [(4, "r4", np.float32), (8, "r8", np.float64)]
CANARY = -7.0
NCOL = 30
OUT = LU.LIDAR_OUT
IN = LU.GRID + ["presf", "land"]


@pytest.fixture(scope="module")
def fx():
    f, g, h = np.load(LU.FIXTURE), np.load(U.FIXTURE), np.load(M.FIXTURE)
    d = {k: f[k] for k in f.files}
    d.update(mask=g["mask_ov3"], t=g["in_at"], reff_lsliq=h["in_rl"], reff_lsice=h["in_ri"], reff_cvliq=h["in_rlc"], reff_cvice=h["in_ric"])
    d["isccp"] = {k: g[k] for k in g.files if k.startswith("in_")}
    d["hydro"] = {k: h[k] for k in h.files if k.startswith("in_")}
    return d


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def _dev(a, dt):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).cuda()


def _shapes(nlev, ncol, npts):
    return {"lidarcld": (nlev, npts), "cldlayer": (4, npts), "cfad_sr": (nlev, 15, npts), "parasolrefl": (5, npts), "pmol": (nlev, npts),
            "beta_tot": (nlev, ncol, npts), "tau_tot": (nlev, ncol, npts), "refl": (5, ncol, npts)}


def dev_lidar(ctx, b, ice, want=OUT, check=True):
    """geosrad_lidar_dev on device copies; an input that is None in `b` is passed as NULL; every output is allocated and canary-filled,
    those in `want` are passed"""
    import torch
    nlev, ncol, npts = b["mask"].shape
    t = {k: _dev(b[k], ctx.dtype) for k in IN if b.get(k) is not None}
    t["frac_out_u8"] = _dev(b["mask"], np.uint8)
    tdt = torch.float32 if ctx.dtype == np.float32 else torch.float64
    o = {k: torch.full(s, CANARY, dtype=tdt, device="cuda") for k, s in _shapes(nlev, ncol, npts).items()}
    ptr = {k: v.data_ptr() for k, v in t.items()}
    ptr.update({k: o[k].data_ptr() for k in want})
    try:
        ctx.lidar_dev(_stream(), npts, nlev, ncol, ice, ptr)
        if check:
            ctx.check(_stream())
    finally:
        torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in o.items()}


def host_args(b, ice, dt):
    nlev, ncol, npts = b["mask"].shape
    return [npts, nlev, ncol, ice, b["p"], b["t"], b["presf"], b["pplay"], b["mask"].astype(dt), *[b[n] for n in LU.GRID[3:]], b["land"]]


@pytest.fixture(scope="module")
def lidar_runs(gpu_ctx, fx):
    return {(rk, ice): dev_lidar(gpu_ctx[rk], batch(fx), ice) for rk, _, _ in KINDS for ice in (0, 1)}


def _cloudy(c):
    return (c >= 4) & (c <= LU.ABOVE)


def _usable(c):
    return (c >= 1) & (c <= LU.ABOVE)


@pytest.mark.gpu
@pytest.mark.parametrize("ice", [0, 1])
@pytest.mark.parametrize("rk,kind,dt", KINDS)
def test_lidar_against_the_reference(lidar_runs, fx, rk, kind, dt, ice):
    got, tag = lidar_runs[(rk, ice)], f"_ice{ice}"
    eps, eps32 = float(np.finfo(dt).eps), float(np.finfo(np.float32).eps)
    undef = dt(LU.R_UNDEF)
    assert all(got[n].dtype == dt for n in OUT)
    # discrete: the bin of every cell from the device's own pnorm and pmol (the division is IEEE in numpy and on the device), the counts
    code, _ = LU.bin_codes(got["beta_tot"], got["pmol"], dt)
    ref = fx[f"{kind}_code{tag}"]
    differ = (code != ref) | (_cloudy(code) != _cloudy(ref)) | (_usable(code) != _usable(ref))
    moved = int(differ.sum())
    cap = 0.002 * ref.size if dt is np.float32 else 0
    print(f"{kind} ice_type {ice}: {moved} of {ref.size} cells with another bin, cloudy or usable decision (cap {cap:.0f})")
    assert moved <= cap, (kind, moved)
    cnt, rcnt = LU.cfad_counts(got["cfad_sr"], NCOL), fx[f"{kind}_cfad_counts{tag}"].astype(np.int64)
    assert np.array_equal(cnt == -1, rcnt == -1), "undefined cfad_sr cells"
    hmoved = int(np.abs(cnt - rcnt).sum() + 1) // 2
    print(f"{kind} ice_type {ice}: {hmoved} sub-columns in another cfad_sr bin; {int((np.where(rcnt > 0, rcnt, 0).sum(axis=(0, 2)) > 0).sum())} of 15 bins populated")
    assert hmoved <= cap
    # the counts are those of the device's own cells, and cfad_sr is count / ncol in the kind
    own = np.stack([(code == b).sum(axis=1) for b in range(15)], axis=1)
    assert np.array_equal(np.where(cnt == -1, own, cnt), own)
    np.testing.assert_array_equal(got["cfad_sr"][cnt != -1], (cnt[cnt != -1].astype(dt) / dt(NCOL)))
    same_lev, same_pt = ~differ.any(axis=1), ~differ.any(axis=(0, 1))
    np.testing.assert_array_equal(got["lidarcld"][same_lev], fx[f"{kind}_lidarcld{tag}"][same_lev])
    np.testing.assert_array_equal(got["cldlayer"][:, same_pt], fx[f"{kind}_cldlayer{tag}"][:, same_pt])
    assert (got["lidarcld"] == undef).sum() >= 70 and ((got["lidarcld"] == undef) == (fx[f"{kind}_lidarcld{tag}"] == undef))[same_lev].all()
    land = fx["in_land"] == 1
    assert (got["parasolrefl"][:, land] == undef).all() and (got["parasolrefl"][:, ~land] != undef).all()
    # continuous
    sample = fx["sample"]
    for n in ("parasolrefl", "pmol", "beta_tot", "tau_tot", "refl"):
        g = got[n][..., sample] if n in ("beta_tot", "tau_tot", "refl") else got[n]
        r = fx[f"{kind}_{n}{tag}"]
        ok = r != undef
        d = np.abs(g.astype(np.float64) - r.astype(np.float64))[ok]
        a = np.abs(r.astype(np.float64))[ok]
        if dt is np.float32:
            spread, floor = float(fx[f"spread_{n}{tag}"]), 4 * eps32 * float(a.max())
            bound = max(4 * spread, floor)
            print(f"{kind} ice_type {ice} {n}: max |dev - ref| = {d.max():.3e} = {d.max() / max(spread, 1e-300):.2f} x the r4-r8 spread {spread:.2e} (bound {bound:.2e})")
            assert d.max() <= bound, (n, float(d.max()), bound)
        else:
            rel = max(64 * eps, 4 * float(fx[f"restate64rel_{n}{tag}"]))
            e = np.where(d == 0, 0, d / np.maximum(a, 1e-300))
            print(f"{kind} ice_type {ice} {n}: max rel = {e.max():.3e} = {e.max() / eps:.1f} eps (bound {rel / eps:.0f} eps)")
            assert (d <= rel * a).all(), (n, float(e.max()))


@pytest.mark.gpu
@pytest.mark.parametrize("rk,kind,dt", KINDS)
def test_optional_outputs_change_no_other_bit(gpu_ctx, lidar_runs, fx, rk, kind, dt):
    got, b = lidar_runs[(rk, 1)], batch(fx)
    for drop in (("beta_tot", "tau_tot", "refl"), ("lidarcld", "pmol"), ("cfad_sr", "cldlayer", "parasolrefl", "tau_tot"), ("parasolrefl",)):
        g = dev_lidar(gpu_ctx[rk], b, 1, want=[n for n in OUT if n not in drop])
        for n in OUT:
            if n in drop:
                assert (g[n] == dt(CANARY)).all(), n
            else:
                np.testing.assert_array_equal(g[n], got[n], err_msg=f"{n} without {drop}")


def _other_batch(npts, ncol, nlev):
    b0 = U.make_batch(npts, nlev, seed=29 + npts + ncol)
    if nlev <= 3:
        rng = np.random.default_rng(nlev)
        on = (np.arange(npts) % 3 != 0)[None, :] & (rng.uniform(0, 1, (nlev, npts)) < 0.7)
        b0["cc"] = np.where(on, rng.uniform(0.2, 1.0, (nlev, npts)), 0).astype(np.float32)
        b0["dtau_s"] = np.where(on, 0.05 * np.exp(5.0 * rng.uniform(0, 1, (nlev, npts))), 0).astype(np.float32)
        b0["conv"] = np.where(on & (np.arange(npts) % 2 == 1)[None, :], 0.5 * b0["cc"], 0).astype(np.float32)
        b0["dtau_c"] = np.where(b0["conv"] > 0, np.float32(2.0), np.float32(0.0)).astype(np.float32)
    hy = LU.thicken(M.make_hydro(b0, seed=5 + nlev), b0)
    ex = LU.make_lidar_inputs(b0)
    mask, _ = U.scops(b0["seed"], b0["cc"], b0["conv"], 3, ncol, np.float32)
    return dict(p=ex["p"], t=b0["at"], presf=ex["presf"], pplay=ex["pplay"], land=ex["land"], mask=mask, mr_lsliq=hy["ql"], mr_lsice=hy["qi"], mr_cvliq=hy["qlc"],
                mr_cvice=hy["qic"], reff_lsliq=hy["rl"], reff_lsice=hy["ri"], reff_cvliq=hy["rlc"], reff_cvice=hy["ric"])


@pytest.mark.gpu
@pytest.mark.parametrize("rk,kind,dt", KINDS)
@pytest.mark.parametrize("npts,ncol,nlev", [(70, 30, 24), (96, 2, 24), (96, 7, 24), (130, 7, 3)])
def test_other_shapes_against_the_restatement(gpu_ctx, rk, kind, dt, npts, ncol, nlev):
    """a partial wavefront of points, more than one block of sub-columns, two, seven and thirty sub-columns, three levels.  Against the
    restatement: no discrete difference; the continuous outputs within 64 eps of the kind or, for the three that hold 1 - exp(-2 tau) of
    a thin layer, 64 eps over that layer's 2 tau (the restatement's exp is the float64 function rounded once, the device's its own).
    NULL for the four convective arrays is explicit zeros bit for bit, also where the mask has convective cells"""
    b = _other_batch(npts, ncol, nlev)
    ice = (npts + ncol) % 2
    want = restate(b, ice, dt)
    got = dev_lidar(gpu_ctx[rk], b, ice)
    eps = float(np.finfo(dt).eps)
    code, _ = LU.bin_codes(got["beta_tot"], got["pmol"], dt)
    print(f"{kind} {npts} x {nlev} x {ncol}: {int((code != want['code']).sum())} of {code.size} cells in another bin; {int(_cloudy(want['code']).sum())} cloudy cells")
    assert _cloudy(want["code"]).sum() > npts // 4 and (want["code"] == 0).any()
    np.testing.assert_array_equal(code, want["code"])
    for n in ("lidarcld", "cldlayer", "cfad_sr", "tau_tot", "refl", "parasolrefl"):
        np.testing.assert_array_equal(got[n], want[n], err_msg=n)
    # 1 - exp(-2 tau) of a layer: an ulp of exp is eps / (2 tau) of the difference.  The layer depths in float64: the sub-columns' from
    # tau_tot, the molecules' from the restatement on a single clear sub-column
    layers = lambda t: np.concatenate([t[:1], np.diff(t, axis=0)])
    clear = (np.zeros((nlev, 1, npts)),) * 4
    tau_mol = LU.simulate(b["p"], b["t"], b["presf"], clear, (b["reff_lsliq"], b["reff_lsice"], b["reff_cvliq"], b["reff_cvice"]), ice, np.float64)[2][:, 0]
    for n, lay in (("beta_tot", layers(want["tau_tot"].astype(np.float64))), ("pmol", layers(tau_mol))):
        w = want[n].astype(np.float64)
        d = np.abs(got[n].astype(np.float64) - w)
        e = d / np.maximum(np.abs(w), 1e-300) / (1.0 + 1.0 / np.maximum(2.0 * lay, 1e-300))
        print(f"{kind} {npts} x {nlev} x {ncol} {n}: max rel / (1 + 1 / (2 tau)) = {e.max() / eps:.2f} eps")
        assert (e <= 64 * eps).all(), (n, float(e.max() / eps))
    nul = dev_lidar(gpu_ctx[rk], dict(b, mr_cvliq=None, mr_cvice=None, reff_cvliq=None, reff_cvice=None), ice)
    zer = dev_lidar(gpu_ctx[rk], dict(b, **{k: np.zeros_like(b["t"]) for k in ("mr_cvliq", "mr_cvice", "reff_cvliq", "reff_cvice")}), ice)
    assert (b["mask"] == 2).any() or nlev > 3
    for n in OUT:
        np.testing.assert_array_equal(nul[n], zer[n], err_msg=n)


@pytest.mark.gpu
@pytest.mark.parametrize("rk,kind,dt", KINDS)
def test_refusals_and_the_range_check(gpu_ctx, fx, rk, kind, dt):
    from geosradiation_gridcomp_amd.api import GeosradError, GeosradInputError
    ctx = gpu_ctx[rk]
    b = batch(fx)
    with pytest.raises(GeosradError, match="ice_type") as e:
        dev_lidar(ctx, b, 2)
    assert e.value.rc == 1
    one = {k: (v[:2] if k == "presf" else v[:1] if getattr(v, "ndim", 0) >= 2 else v) for k, v in b.items()}
    with pytest.raises(GeosradError, match="nlev") as e:
        dev_lidar(ctx, one, 0)
    assert e.value.rc == 1
    for name in ("p", "presf", "pplay", "reff_lsice", "land"):
        with pytest.raises(GeosradError, match="null") as e:
            dev_lidar(ctx, dict(b, **{name: None}), 0)
        assert e.value.rc == 1
    bad = dict(b, t=b["t"].copy()); bad["t"][40, 17] = 0.0
    with pytest.raises(GeosradInputError, match=r"\): t$") as e:
        dev_lidar(ctx, bad, 0)
    assert e.value.rc == 5
    ctx.check(_stream())                        # reported once; the flag is down again
    bad = dict(b, p=b["p"].copy()); bad["p"][3, 90] = -1.0
    with pytest.raises(GeosradInputError, match=r"\): p$") as e:          # the host variant returns it itself
        ctx.lidar(*host_args(bad, 0, dt))
    assert e.value.rc == 5
    ctx.check(_stream())


@pytest.mark.gpu
@pytest.mark.parametrize("rk,kind,dt", KINDS)
def test_host_variant_equals_the_device_one_across_chunks_and_shards(gpu_ctx, lidar_runs, fx, rk, kind, dt):
    from geosradiation_gridcomp_amd.api import Context
    ctx = gpu_ctx[rk]
    b = {k: np.ascontiguousarray(np.concatenate([v, v[..., ::-1]], axis=-1)) for k, v in batch(fx).items()}
    dev = dev_lidar(ctx, b, 0)
    args = host_args(b, 0, dt)
    ctx.set_chunk(64)
    try:
        host = ctx.lidar(*args, want=OUT)
    finally:
        ctx.set_chunk(131072)
    multi = Context(rk, devices=[0, 0], tables=False)
    try:
        shard = multi.lidar(*args, want=OUT)
    finally:
        multi.close()
    for n in OUT:
        np.testing.assert_array_equal(host[n], dev[n], err_msg=n)
        np.testing.assert_array_equal(shard[n], dev[n], err_msg="sharded " + n)
        np.testing.assert_array_equal(dev[n][..., :96], lidar_runs[(rk, 0)][n], err_msg=n)


@pytest.mark.gpu
@pytest.mark.parametrize("rk,kind,dt", KINDS)
@pytest.mark.parametrize("conv", [True, False])
def test_cosp_lidar_dev(gpu_ctx, fx, rk, kind, dt, conv):
    """geosrad_cosp_lidar_dev on satsim_util.model_fields plus MODIS's planes and FROCEAN: its first outputs, the seeds and SGFCLD equal
    geosrad_cosp_dev's bit for bit, its lidar outputs geosrad_lidar_dev on numpy-prepared arrays (the shifted presf, pplay = ph, a negative
    QLTOT clamped, the land rule) bit for bit, in model order; with the five lidar outputs NULL nothing else changes"""
    import torch
    from tests.test_gpu_satsim import dev_scops
    ctx = gpu_ctx[rk]
    f = U.model_fields({k[3:]: v for k, v in fx["isccp"].items() if k != "in_emsfc_lw"})
    if not conv:
        f["CCA"] = f["DTAU_C"] = f["DEM_C"] = None
    lm, npts = f["T"].shape
    hyd = fx["hydro"]
    rng = np.random.default_rng(13)
    zsfc = rng.uniform(0., 1500., npts)
    zle = np.concatenate([(hyd["in_zfull"][0] + 900.)[None, :], 0.5 * (hyd["in_zfull"][:-1] + hyd["in_zfull"][1:]), np.zeros((1, npts))]) + zsfc[None, :]
    new = dict(ZLE=zle.astype(np.float32), QLTOT=hyd["in_ql"].copy(), QITOT=hyd["in_qi"], RDFL=hyd["in_rl"], RDFI=hyd["in_ri"])
    new["QLTOT"][new["QLTOT"] > 0] *= np.where(rng.uniform(0, 1, int((new["QLTOT"] > 0).sum())) < 0.3, -1, 1).astype(np.float32)      # some negative: clamped
    frocean = np.where(np.arange(npts) % 4 == 0, 0.5, rng.uniform(0, 1, npts)).astype(np.float32)      # 0.5 itself is ocean
    names = ["T", "QV", "FCLD", "CCA", "PLE", "PLO", "DTAU_S", "EMISS", "DTAU_C", "DEM_C", "TS"]
    cosp_out = list(ctx.ICARUS_OUT) + ["SGFCLD"] + list(M.MISR_OUT) + ["modis_mean", "modis_hist"]
    lidar_out = ["clcalipso", "cldlayer", "cfad_sr", "parasolrefl", "lidarpmol"]
    shapes = {"fq_isccp": (7, 7, npts), "boxtau": (NCOL, npts), "boxptop": (NCOL, npts), "SGFCLD": (lm, npts), "fq_MISR_TAU_v_CTH": (16, 7, npts),
              "dist_model_layertops": (16, npts), "modis_mean": (17, npts), "modis_hist": (7, 7, npts), "clcalipso": (lm, npts), "cldlayer": (4, npts),
              "cfad_sr": (lm, 15, npts), "parasolrefl": (5, npts), "lidarpmol": (lm, npts)}

    def run(entry, skip=()):
        t = {k: _dev(f[k], dt) for k in names if f[k] is not None}
        t.update({k: _dev(v, dt) for k, v in new.items()})
        t["FROCEAN"] = _dev(frocean, dt)
        t["sunlit"] = _dev(f["sunlit"], np.int32); t["seed"] = _dev(f["seed"], np.int32)
        o = {k: torch.full(shapes.get(k, (npts,)), CANARY, dtype=t["TS"].dtype, device="cuda") for k in cosp_out + lidar_out}
        ptr = {k: v.data_ptr() for k, v in t.items()}
        ptr.update({k: v.data_ptr() for k, v in o.items() if k not in skip})
        if entry == "cosp":
            ctx.cosp_dev(_stream(), npts, lm, NCOL, {k: v for k, v in ptr.items() if k not in lidar_out + ["FROCEAN"]}, emsfc_lw=U.EMSFC_LW)
        else:
            ctx.cosp_lidar_dev(_stream(), npts, lm, NCOL, ptr, emsfc_lw=U.EMSFC_LW, ice_type=0)
        ctx.check(_stream()); torch.cuda.synchronize()
        return {k: v.cpu().numpy() for k, v in o.items()}, t["seed"].cpu().numpy()

    base, bseed = run("cosp")
    got, seed = run("lidar")
    np.testing.assert_array_equal(seed, bseed)
    for n in cosp_out:
        np.testing.assert_array_equal(got[n], base[n], err_msg=n)
    # geosrad_lidar_dev on what numpy prepares as the GridComp and COSP do
    z = np.zeros_like(np.asarray(f["FCLD"], dt))
    mask, _ = dev_scops(ctx, f["seed"], np.asarray(f["FCLD"], dt), z if f["CCA"] is None else np.asarray(f["CCA"], dt), 3, NCOL)
    pre = LU.cosp_lidar_prepare(f, new, frocean, dt)
    assert (pre["land"] == 1).any() and (pre["land"][::4] == 0).all() and (new["QLTOT"] < 0).sum() > 20 and (pre["presf"][0] == 0).all()
    ref = dev_lidar(ctx, dict(pre, mask=mask), 0, want=["lidarcld", "cldlayer", "cfad_sr", "parasolrefl", "pmol"])
    for n, m in zip(lidar_out, ["lidarcld", "cldlayer", "cfad_sr", "parasolrefl", "pmol"]):
        np.testing.assert_array_equal(got[n], ref[m], err_msg=n)
    assert ((got["clcalipso"] > 0) & (got["clcalipso"] != dt(LU.R_UNDEF))).sum() > 40
    # a level's row is the model's: the top level of pmol is the thin layer between 0 and PLE(0), the smallest signal of its column
    assert (got["lidarpmol"][0] < got["lidarpmol"][-1]).all()
    # with the five lidar outputs NULL nothing else changes and the lidar's arrays are untouched; a part of them wanted changes no other bit
    part, pseed = run("lidar", skip=lidar_out)
    np.testing.assert_array_equal(pseed, bseed)
    for n in cosp_out:
        np.testing.assert_array_equal(part[n], base[n], err_msg=n)
    for n in lidar_out:
        assert (part[n] == dt(CANARY)).all(), n
    part, _ = run("lidar", skip=["cfad_sr", "lidarpmol", "modis_mean", "modis_hist"] + list(M.MISR_OUT))
    for n in cosp_out + lidar_out:
        if n in ("cfad_sr", "lidarpmol", "modis_mean", "modis_hist") or n in M.MISR_OUT:
            assert (part[n] == dt(CANARY)).all(), n
        else:
            np.testing.assert_array_equal(part[n], got[n], err_msg=n)
