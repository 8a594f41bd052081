"""Helpers of tests/test_sw_cldhb.py: GEOS-native fields for the heartbeat McICA cloud fractions (CLD??SWHB, GEOS_SolarGridComp.F90:7060-7223),
a numpy restatement of the block's preparation (:7133-7161) in a given dtype - numpy rounds every operation on its own, so it is un-fused -
and the four exports from it through a generator + clearCounts_threeBand of the caller's choice."""
import numpy as np

NSUB = 112                       # ngptsw
SEED_ORDER = (4, 3, 2, 1)        # :7179
GRAV, RGAS = 9.80665, 8314.47 / 28.965      # MAPL_GRAV, MAPL_RGAS = MAPL_RUNIV / MAPL_AIRMW
OUT = ["CLDTT", "CLDHI", "CLDMD", "CLDLO"]


def make_fields(ncol, lm, seed, clear=0.3):
    """FCLD, T, QI, QL (lm, ncol), PLE (lm + 1, ncol) in Pa increasing with the index (TOA first), LATS (ncol) in radians over both
    hemispheres, float64; and LCLDMH / LCLDLM (the first layers below 400 / 700 hPa of a 1000 hPa column).  A `clear` share of the columns
    has no cloud fraction (some of them condensate all the same); the others one to three decks with fractions that reach every branch
    of the generator's sigma (<= 0.9, > 0.9, > 0.99, 1), cloudy layers without or with negligible condensate, and condensate outside
    the decks."""
    rng = np.random.default_rng(seed)
    eta = np.linspace(0.0, 1.0, lm + 1) ** 2.2
    ps = rng.uniform(94000.0, 103500.0, ncol)
    ple = 1.0 + eta[:, None] * (ps - 1.0)[None, :]
    pm = 0.5 * (ple[:-1] + ple[1:])
    t = 205.0 + 85.0 * (pm / ps) ** 0.6 + rng.normal(0.0, 1.5, (lm, ncol))
    fcld = np.zeros((lm, ncol))
    for i in range(ncol):
        for _ in range(int(rng.integers(1, 4))):
            top = int(rng.integers(lm // 6, lm - 1))
            bot = min(lm, top + int(rng.integers(1, max(2, lm // 8))))
            kind = rng.uniform()
            f = 1.0 if kind < 0.1 else rng.uniform(0.991, 0.9999) if kind < 0.2 else rng.uniform(0.9, 0.99) if kind < 0.3 else rng.uniform(0.02, 0.9)
            fcld[top:bot, i] = np.maximum(fcld[top:bot, i], f * rng.uniform(0.6, 1.0, bot - top) if f < 0.9 else f)
    warm = t > 255.0
    ql = np.where(warm, 10.0 ** rng.uniform(-6.0, -3.3, (lm, ncol)), 0.0) * (rng.uniform(0, 1, (lm, ncol)) < 0.8)
    qi = np.where(t < 270.0, 10.0 ** rng.uniform(-7.0, -4.0, (lm, ncol)), 0.0) * (rng.uniform(0, 1, (lm, ncol)) < 0.8)
    none = rng.uniform(0, 1, (lm, ncol)) < 0.08                # cloudy layers without condensate: the cwp_tiny reset
    ql[none] = 0.0; qi[none] = 0.0
    tiny = rng.uniform(0, 1, (lm, ncol)) < 0.05                # condensate whose water path lies either side of cwp_tiny = 1e-20
    ql[tiny] = 10.0 ** rng.uniform(-26.0, -22.0, int(tiny.sum())); qi[tiny] = 0.0
    fcld[:, rng.uniform(0, 1, ncol) < clear] = 0.0
    lats = rng.uniform(-0.5 * np.pi, 0.5 * np.pi, ncol)
    pref = 1.0 + eta * (100000.0 - 1.0)
    pmr = 0.5 * (pref[:-1] + pref[1:])
    lcldmh = min(max(int(np.argmax(pmr > 40000.0)) + 1, 2), lm - 1)
    lcldlm = min(max(int(np.argmax(pmr > 70000.0)) + 1, lcldmh + 1), lm)
    assert 1 < lcldmh < lcldlm <= lm
    return dict(FCLD=fcld, PLE=ple, T=t, QI=qi, QL=ql, LATS=lats), lcldmh, lcldlm


def prepare(f, dt, grav=GRAV, rgas=RGAS):
    """the generator's inputs as SOL:7133-7161 forms them, statement by statement in dtype dt, for ALL columns of f: zmid, play, cldfrac,
    ciwp, clwp (lm, ncol), alat (ncol); TOA first, as the reference leaves them (:7125-7131)"""
    dt = np.dtype(dt).type
    ple, t = f["PLE"].astype(dt), f["T"].astype(dt)
    qi, ql = f["QI"].astype(dt), f["QL"].astype(dt)
    lm = t.shape[0]
    g, r = dt(grav), dt(rgas)
    plmid = dt(0.5) * (ple[:-1] + ple[1:])
    play = plmid / dt(100.)
    cfac = (dt(1.02) * dt(100)) * (ple[1:] - ple[:-1])
    ciwp, clwp = cfac * qi, cfac * ql
    tlev = (t[:-1] * cfac[1:] + t[1:] * cfac[:-1]) / (cfac[1:] + cfac[:-1])
    zmid = np.zeros_like(t)
    for k in range(lm - 2, -1, -1):
        zmid[k] = zmid[k + 1] + (((r * tlev[k]) / g) * (plmid[k + 1] - plmid[k])) / ple[k + 1]
    for a in (plmid, play, cfac, ciwp, clwp, tlev, zmid):
        assert a.dtype == np.dtype(dt)
    return dict(zmid=zmid, play=play, cldfrac=f["FCLD"].astype(dt), ciwp=ciwp, clwp=clwp, alat=f["LATS"].astype(dt))


def cloudy_columns(f):
    return np.flatnonzero((f["FCLD"] > 0).any(axis=0))


def clear_counts(p, cols, doy, lcldmh, lcldlm, how, kind=None, ctx=None):
    """clearCounts (len(cols), 4) of generate_stochastic_clouds(112 sub-columns, seed_order [4,3,2,1], cwp_tiny 1e-20) +
    clearCounts_threeBand(cloudLM = lcldlm, cloudMH = lcldmh) on the columns `cols` of prepare()'s arrays, as the reference feeds its
    cloudy columns only.  how: "reflib" (the reference's Fortran, kind r4 / r8), "clib" (the oracle, kind r4 / r8), "device" (ctx's
    generate_stochastic_clouds_dev + clearCounts_threeBand).  The condensate inhomogeneity is whatever the caller has set there."""
    s = {k: np.ascontiguousarray(v[..., cols]) for k, v in p.items()}
    lm, n = s["play"].shape
    if n == 0:
        return np.zeros((0, 4), dtype=np.int32)
    if how == "reflib":
        from oracle import reflib
        cldy = reflib.mcica(s["zmid"], s["alat"], doy, s["play"], s["cldfrac"], s["ciwp"], s["clwp"], NSUB, seed_order=SEED_ORDER, kind=kind)[0]
        return reflib.clearcounts(cldy, lcldlm, lcldmh, kind=kind)
    if how == "clib":
        from oracle import clib
        cldy = clib.mcica(s["zmid"], s["alat"], doy, s["play"], s["cldfrac"], s["ciwp"], s["clwp"], NSUB, seed_order=SEED_ORDER, prec=kind)[0]
        return clib.clearcounts(cldy, lcldlm, lcldmh)
    assert how == "device"
    import torch
    tdt = torch.float32 if ctx.dtype == np.float32 else torch.float64
    names = dict(zm="zmid", alat="alat", play="play", cldf="cldfrac", ciwp="ciwp", clwp="clwp")
    d = {k: torch.from_numpy(np.ascontiguousarray(s[v], dtype=ctx.dtype)).cuda() for k, v in names.items()}
    d["cldy_stoch"] = torch.zeros((n, NSUB, lm), dtype=torch.int32, device="cuda")
    d["ciwp_stoch"] = torch.zeros((n, NSUB, lm), dtype=tdt, device="cuda")
    d["clwp_stoch"] = torch.zeros((n, NSUB, lm), dtype=tdt, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    ctx.generate_stochastic_clouds_dev(st, n, NSUB, lm, {k: v.data_ptr() for k, v in d.items()}, doy, 1e-20, seed_order=SEED_ORDER)
    ctx.check(st)
    return ctx.clearCounts_threeBand(n, NSUB, lm, lcldlm, lcldmh, d["cldy_stoch"].cpu().numpy())


def exports(f, dt, doy, lcldmh, lcldlm, how, kind=None, ctx=None, p=None):
    """CLDTT, CLDHI, CLDMD, CLDLO (4, ncol) in dtype dt: 1 - count / 112 on the columns with cloud fraction (:7187-7206), 0 elsewhere
    (:7077-7080); and the counts (4, ncol), 112 where nothing was generated"""
    dt = np.dtype(dt).type
    p = prepare(f, dt) if p is None else p
    cols = cloudy_columns(f)
    ncol = f["FCLD"].shape[1]
    cnt = np.full((4, ncol), NSUB, dtype=np.int32)
    cnt[:, cols] = clear_counts(p, cols, doy, lcldmh, lcldlm, how, kind=kind, ctx=ctx).T
    out = np.zeros((4, ncol), dtype=dt)
    out[:, cols] = dt(1.) - cnt[:, cols].astype(dt) / dt(NSUB)
    return out, cnt
