"""Helpers of the satellite-simulator tests: the batch recipe of tests/golden/satsim_isccp_72.npz and a numpy restatement of
GEOSsatsim_GridComp's scops.f (+ congvec.f), icarus.f, the wrapper of cosp_isccp_simulator.F90:58-90 and the seed rule of cosp.F90:167-174,
statement by statement in the real kind it is given - numpy rounds every operation on its own, so it is un-fused.

Layouts as everywhere in the tests: C order with the point index last, i.e. the reference's Fortran arrays with the point index first:
cc (nlev, npoints), frac_out (nlev, ncol, npoints), boxtau (ncol, npoints), fq_isccp (7 pressure, 7 tau, npoints)."""
import os

import numpy as np

MISSING = -1.0e30
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "satsim_isccp_72.npz")
ICARUS_OUT = ["fq_isccp", "totalcldarea", "meanptop", "meantaucld", "meanalbedocld", "meantb", "meantbclr", "boxtau", "boxptop"]
CONTINUOUS = ICARUS_OUT[1:]
OPTION_PAIRS = [(th, thd) for th in (1, 2, 3) for thd in (1, 2)]
IN_2D = ["pfull", "phalf", "qv", "cc", "conv", "dtau_s", "dtau_c", "at", "dem_s", "dem_c"]
EMSFC_LW = 0.999         # GEOS_SatsimGridComp.F90:3462


def make_batch(npoints=96, nlev=72, seed=20261, dtype=np.float32):
    """The fixture's inputs (the defaults) or a batch of another size by the same recipe, TOA first as scops / icarus take them, every
    real already rounded to float32 so that the r4 and the r8 build of the reference read the same numbers.  phalf = ps exp(-9.2 (nlev+1-k)
    / nlev) + 1 Pa with phalf(1) = 0; a temperature profile without two equal neighbouring levels (a power law up to 200 hPa, strictly
    warming above, a per-point offset, and in a third of the points a layer 14 K colder at 0.83 ps under an inversion, so that a
    brightness temperature matches at several levels and the two search directions differ); cloud decks below 150 hPa in a quarter of
    the layers, cc in 0.05-1, dtau_s = 0.02 e^(7.5 u),
    dem_s = 1 - e^(-dtau_s / 2); convective cloud with its own optics in every third point; one point in eight cloud-free, one in four
    dark; skt within -2..+4 K of the lowest level; seeds spread over 1..100 001."""
    rng = np.random.default_rng(seed)
    ps = rng.uniform(96000.0, 103000.0, npoints)
    k = np.arange(1, nlev + 2)[:, None]
    phalf = ps[None, :] * np.exp(-9.2 * (nlev + 1 - k) / nlev) + 1.0
    phalf[0] = 0.0
    pfull = 0.5 * (phalf[:-1] + phalf[1:])
    tsfc = 288.0 + rng.uniform(-12.0, 12.0, npoints)
    t200 = tsfc * (20000.0 / ps) ** 0.19
    at = np.where(pfull >= 20000.0, tsfc[None, :] * (pfull / ps[None, :]) ** 0.19, t200[None, :] + 9.0 * np.log(20000.0 / np.minimum(pfull, 20000.0)))
    at = at - np.where((np.arange(npoints) % 3 == 2)[None, :], 14.0 * np.exp(-((pfull / ps[None, :] - 0.83) / 0.05) ** 2), 0.0)
    qv = 0.015 * (pfull / ps[None, :]) ** 3 + 3.0e-6
    deck = (rng.uniform(0, 1, (nlev, npoints)) < 0.25) & (pfull > 15000.0)
    cc = np.where(deck, rng.uniform(0.05, 1.0, (nlev, npoints)), 0.0)
    dtau_s = np.where(deck, 0.02 * np.exp(7.5 * rng.uniform(0, 1, (nlev, npoints))), 0.0)
    dem_s = np.where(deck, 1.0 - np.exp(-0.5 * dtau_s), 0.0)
    j = np.arange(npoints)
    cdeck = deck & (rng.uniform(0, 1, (nlev, npoints)) < 0.5) & (j % 3 == 1)[None, :]
    conv = np.where(cdeck, cc * rng.uniform(0.1, 0.9, (nlev, npoints)), 0.0)
    dtau_c = np.where(cdeck, 0.05 * np.exp(6.0 * rng.uniform(0, 1, (nlev, npoints))), 0.0)
    dem_c = np.where(cdeck, 1.0 - np.exp(-0.5 * dtau_c), 0.0)
    clear = (j % 8 == 5)[None, :]
    for a in (cc, conv, dtau_s, dtau_c, dem_s, dem_c):
        a[np.broadcast_to(clear, a.shape)] = 0.0
    b = dict(pfull=pfull, phalf=phalf, qv=qv, cc=cc, conv=conv, dtau_s=dtau_s, dtau_c=dtau_c, at=at, dem_s=dem_s, dem_c=dem_c,
             skt=at[-1] + rng.uniform(-2.0, 4.0, npoints))
    b = {n: np.ascontiguousarray(v.astype(np.float32).astype(dtype)) for n, v in b.items()}
    b["sunlit"] = (j % 4 != 3).astype(np.int32)
    b["seed"] = (1 + (j * 100000) // max(npoints - 1, 1) if npoints > 1 else np.array([4711])).astype(np.int32)
    assert (np.diff(b["at"].astype(np.float32), axis=0) != 0).all()
    return b


# exp, log and the powers of the real kind: the float64 function rounded once, which is what a correctly rounded expf / logf / powf gives
# in all but the rarest cases (numpy's own float32 loops are SIMD approximations good to a few ulp, further from the reference's libm)
def _exp(x):
    return np.exp(np.asarray(x, np.float64)).astype(np.asarray(x).dtype)


def _log(x):
    return np.log(np.asarray(x, np.float64)).astype(np.asarray(x).dtype)


def _pow(x, y):
    return np.power(np.asarray(x, np.float64), np.float64(y)).astype(np.asarray(x).dtype)


# ---- scops.f + congvec.f ------------------------------------------------------------------------------------------------------------
def congvec(seed, R):
    """congvec.f:37-52 for every point: `seed` (int32, updated in place) and the draw in the real kind"""
    t = 69069 * seed.astype(np.int64) + 1234567
    t = ((t + 2 ** 31) % 2 ** 32) - 2 ** 31                  # the 32-bit integer wraps
    seed[:] = np.fmod(t, 2 ** 30).astype(np.int32)           # Fortran mod: the dividend's sign
    ran = seed.astype(R) * R(0.931322574615479E-09)
    ran = ran + R(1)                                         # overflow_32 = i2_16*i2_16 wraps to 0 <= huge32: the branch is taken
    return ran - np.trunc(ran).astype(R)


def scops(seed, cc, conv, overlap, ncol, dtype):
    """scops.f: (frac_out uint8 (nlev, ncol, npoints), the seeds as the routine leaves them)"""
    R = np.dtype(dtype).type
    cc, conv = np.asarray(cc, dtype=R), np.asarray(conv, dtype=R)
    nlev, npts = cc.shape
    seed = np.array(seed, dtype=np.int32)
    boxpos = [np.full(npts, (R(ibox) - R(.5)) / R(ncol), dtype=R) for ibox in range(1, ncol + 1)]
    frac_out = np.zeros((nlev, ncol, npts), np.uint8)
    tca = np.concatenate([np.zeros((1, npts), R), cc])
    threshold = [None] * ncol
    one = R(1)
    for ilev in range(1, nlev + 1):
        cv = conv[ilev - 1]
        if ilev == 1:
            for ibox in range(ncol):
                if overlap == 1:
                    threshold[ibox] = boxpos[ibox].copy()
                else:
                    ran = congvec(seed, R)
                    threshold[ibox] = cv + (one - cv) * ran
        for ibox in range(ncol):
            maxocc = (boxpos[ibox] <= cv).astype(R)
            if overlap == 1:
                threshold_min, maxosc = cv, np.ones(npts, R)
            elif overlap == 2:
                threshold_min, maxosc = cv, np.zeros(npts, R)
            else:
                mn = np.minimum(tca[ilev - 1], tca[ilev])
                threshold_min = np.maximum(cv, mn)
                maxosc = ((threshold[ibox] < mn) & (threshold[ibox] > cv)).astype(R)
            ran = congvec(seed, R)
            threshold[ibox] = maxocc * boxpos[ibox] + (one - maxocc) * (
                maxosc * threshold[ibox] + (one - maxosc) * (threshold_min + (one - threshold_min) * ran))
        for ibox in range(ncol):
            f = (tca[ilev] > threshold[ibox]).astype(np.uint8)
            frac_out[ilev - 1, ibox] = np.where(threshold[ibox] <= cv, 2, f)
    return frac_out, seed


# ---- icarus.f -----------------------------------------------------------------------------------------------------------------------
def range_check(cc, conv, dtau_s, dtau_c, dem_s, dem_c):
    """icarus.f:403-455: True where the reference STOPs"""
    bad = (cc < 0) | (cc > 1) | (conv < 0) | (conv > 1) | (dtau_s < 0) | (dtau_c < 0) | (dem_s < 0) | (dem_s > 1) | (dem_c < 0) | (dem_c > 1)
    return bool(np.any(bad))


def icarus(sunlit, pfull, phalf, qv, cc, conv, dtau_s, dtau_c, top_height, top_height_direction, overlap, frac_out, skt, emsfc_lw, at,
           dem_s, dem_c, dtype, detail=False):
    """icarus.f without its printing: a dict of ICARUS_OUT (+ with `detail` the per-sub-column itau, ipres (ncol, npoints), 0 = not binned)"""
    R = np.dtype(dtype).type
    A = lambda x: np.asarray(x, dtype=R)
    pfull, phalf, qv, cc, conv, dtau_s, dtau_c, at, dem_s, dem_c, skt = map(A, (pfull, phalf, qv, cc, conv, dtau_s, dtau_c, at, dem_s, dem_c, skt))
    emsfc_lw = R(emsfc_lw)
    sunlit = np.asarray(sunlit)
    nlev, npts = pfull.shape
    ncol = frac_out.shape[1]
    if range_check(cc, conv, dtau_s, dtau_c, dem_s, dem_c):
        raise ValueError("Input variable out of range")
    one, zero, miss = R(1), R(0), R(MISSING)
    tauchk = R(-1.) * _log(R(0.9999999))
    rec2p13 = one / R(2.13)
    isccp_taumin = R(0.3)
    adj = top_height in (1, 3)
    with np.errstate(all="ignore"):
        if adj:      # :354-384
            ptrop = np.full(npts, 5000., R); attropmin = np.full(npts, 400., R); atmax = np.zeros(npts, R); attrop = np.full(npts, 120., R)
            itrop = np.ones(npts, np.int64)
            for ilev in range(1, nlev + 1):
                m = (pfull[ilev - 1] < R(40000.)) & (pfull[ilev - 1] > R(5000.)) & (at[ilev - 1] < attropmin)
                ptrop = np.where(m, pfull[ilev - 1], ptrop); attropmin = np.where(m, at[ilev - 1], attropmin)
                attrop = np.where(m, attropmin, attrop); itrop = np.where(m, ilev, itrop)
            for ilev in range(1, nlev + 1):
                m = (at[ilev - 1] > atmax) & (ilev >= itrop)
                atmax = np.where(m, at[ilev - 1], atmax)
            meantb = np.zeros(npts, R); meantbclr = np.zeros(npts, R)
        else:
            meantb = np.full(npts, miss, R); meantbclr = np.full(npts, miss, R)
        # :467-492
        tau = np.zeros((ncol, npts), R)
        boxtau = np.full((ncol, npts), miss, R); boxptop = np.full((ncol, npts), miss, R)
        for ilev in range(nlev):
            tau = np.where(frac_out[ilev] == 1, tau + dtau_s[ilev][None, :], tau)
            tau = np.where(frac_out[ilev] == 2, tau + dtau_c[ilev][None, :], tau)
        tb = np.zeros((ncol, npts), R)
        if adj:      # :522-869
            wtmair, wtmh20, Navo, grav, pstd, t0 = R(28.9644), R(18.01534), R(6.023E+23), R(9.806650E+02), R(1.013250E+06), R(296.)
            dem_wv = np.zeros((nlev, npts), R)
            for ilev in range(nlev):
                press = pfull[ilev] * R(10.)
                dpress = (phalf[ilev + 1] - phalf[ilev]) * R(10)
                atmden = dpress / grav
                rvh20 = qv[ilev] * wtmair / wtmh20
                wk = rvh20 * Navo * atmden / wtmair
                rhoave = (press / pstd) * (t0 / at[ilev])
                rh20s = rvh20 * rhoave
                rfrgn = rhoave - rh20s
                tmpexp = _exp(R(-0.02) * (at[ilev] - t0))
                tauwv = wk * R(1.e-20) * ((R(0.0224697) * rh20s * tmpexp) + (R(3.41817e-7) * rfrgn)) * R(0.98)
                dem_wv[ilev] = one - _exp(R(-1.) * tauwv)
            fluxtop_clrsky = np.zeros(npts, R); trans_clr = np.ones(npts, R)
            for ilev in range(nlev):
                bb = one / (_exp(R(1307.27) / at[ilev]) - one)
                fluxtop_clrsky = fluxtop_clrsky + dem_wv[ilev] * bb * trans_clr
                trans_clr = trans_clr * (one - dem_wv[ilev])
            bb = one / (_exp(R(1307.27) / skt) - one)
            fluxtop_clrsky = fluxtop_clrsky + emsfc_lw * bb * trans_clr
            meantbclr = R(1307.27) / (_log(one + (one / fluxtop_clrsky)))
            fluxtop = np.zeros((ncol, npts), R); trans = np.ones((ncol, npts), R)
            for ilev in range(nlev):
                bb = one / (_exp(R(1307.27) / at[ilev]) - one)
                wv = dem_wv[ilev][None, :]
                dem = np.where(frac_out[ilev] == 1, one - ((one - wv) * (one - dem_s[ilev][None, :])),
                               np.where(frac_out[ilev] == 2, one - ((one - wv) * (one - dem_c[ilev][None, :])), wv)).astype(R)
                fluxtop = fluxtop + dem * bb[None, :] * trans
                trans = trans * (one - dem)
            bb = one / (_exp(R(1307.27) / skt) - one)
            fluxtop = fluxtop + emsfc_lw * bb[None, :] * trans
            for ibox in range(ncol):
                meantb = meantb + R(1307.27) / (_log(one + (one / fluxtop[ibox])))
            meantb = meantb / R(ncol)
            btcmin = one / (_exp(R(1307.27) / (attrop - R(5.))) - one)
            for ibox in range(ncol):
                den = fluxtop_clrsky - btcmin
                transmax = np.where(den != zero, (fluxtop[ibox] - btcmin) / np.where(den != zero, den, one), one).astype(R)
                tauir = tau[ibox] * rec2p13
                taumin = R(-1.) * _log(np.maximum(np.minimum(transmax, R(0.9999999)), R(0.001)))
                inr = (transmax > R(0.001)) & (transmax <= R(0.9999999))
                ft = fluxtop[ibox].copy()
                if top_height == 1:
                    fluxtopinit = ft.copy()
                    for _ in range(2):
                        m = (tau[ibox] > tauchk) & inr
                        emcld = one - _exp(R(-1.) * tauir)
                        f2 = fluxtopinit - ((one - emcld) * fluxtop_clrsky)
                        f2 = np.maximum(R(1.E-06), (f2 / emcld))
                        ft = np.where(m, f2, ft).astype(R)
                        tbx = R(1307.27) / (_log(one + (one / ft)))
                        tauir = np.where(m & (tbx > R(260.)), tau[ibox] / R(2.56), tauir).astype(R)
                cloudy = tau[ibox] > tauchk
                t_c = R(1307.27) / (_log(one + (one / ft)))
                low = cloudy & (top_height == 1) & (tauir < taumin)
                t_c = np.where(low, attrop - R(5.), t_c)
                tau[ibox] = np.where(low, R(2.13) * taumin, tau[ibox])
                tb[ibox] = np.where(cloudy, t_c, meantbclr)
        # :930-1008
        ptop = np.zeros((ncol, npts), R)
        for ibox in range(ncol):
            if adj:
                nmatch = np.zeros(npts, np.int64); last = np.zeros(npts, np.int64)
                for k1 in range(1, nlev):
                    ilev = nlev - k1 if top_height_direction == 2 else k1
                    a1, a2, t = at[ilev - 1], at[ilev], tb[ibox]
                    m = (ilev >= itrop) & (((a1 >= t) & (a2 <= t)) | ((a1 <= t) & (a2 >= t)))
                    nmatch = nmatch + m; last = np.where(m, ilev, last)
                jj = np.arange(npts)
                k1 = np.maximum(last, 1) - 1          # 0-based; only used where nmatch >= 1
                k2 = k1 + 1
                logp1 = _log(pfull[k1, jj]); logp2 = _log(pfull[k2, jj])
                atd = np.maximum(tauchk, np.abs(at[k2, jj] - at[k1, jj]))
                logp = logp1 + (logp2 - logp1) * np.abs(tb[ibox] - at[k1, jj]) / atd
                pm = _exp(logp)
                p = np.where(tb[ibox] <= attrop, ptrop, zero)
                p = np.where(tb[ibox] >= atmax, pfull[nlev - 1], p)
                ptop[ibox] = np.where(nmatch >= 1, pm, p)
            else:
                p = np.zeros(npts, R)
                for ilev in range(nlev):
                    p = np.where((p == zero) & (frac_out[ilev, ibox] != 0), phalf[ilev], p)
                ptop[ibox] = p
            ptop[ibox] = np.where(tau[ibox] <= tauchk, zero, ptop[ibox])
        # :1037-1191
        lit = (sunlit == 1) | (top_height == 3)
        fq = np.where(lit[None, None, :], zero, miss) * np.ones((7, 7, npts), R)
        totalcldarea = np.where(lit, zero, miss).astype(R); meanalbedocld = totalcldarea.copy(); meanptop = totalcldarea.copy()
        meantaucld = totalcldarea.copy()
        boxarea = one / R(ncol)
        itau_all = np.zeros((ncol, npts), np.int64); ipres_all = np.zeros((ncol, npts), np.int64)
        taub = [0.3, 1.3, 3.6, 9.4, 23., 60.]
        prb = [180., 310., 440., 560., 680., 800.]
        jj = np.arange(npts)
        for ibox in range(ncol):
            t = tau[ibox]
            cloudy = (t > tauchk) & (ptop[ibox] > zero)
            on = cloudy & lit
            boxtau[ibox] = np.where(on, t, boxtau[ibox])
            thick = on & (t >= isccp_taumin)
            totalcldarea = np.where(thick, totalcldarea + boxarea, totalcldarea)
            albedocld = _pow(t, R(0.895)) / (_pow(t, R(0.895)) + R(6.82))
            meanalbedocld = np.where(thick, meanalbedocld + albedocld * boxarea, meanalbedocld)
            p = ptop[ibox] / R(100.)
            boxptop[ibox] = np.where(on, p, boxptop[ibox])
            meanptop = np.where(thick, meanptop + p * boxarea, meanptop)
            itau = 1 + sum((t >= R(b)).astype(np.int64) for b in taub)
            ipres = np.where(p > zero, 1 + sum((p >= R(b)).astype(np.int64) for b in prb), 0)
            hit = on & (ipres > 0)
            itau_all[ibox] = np.where(hit, itau, 0); ipres_all[ibox] = np.where(hit, ipres, 0)
            for j in jj[hit]:
                fq[ipres[j] - 1, itau[j] - 1, j] = fq[ipres[j] - 1, itau[j] - 1, j] + boxarea
        has = totalcldarea > zero
        safe = np.where(has, totalcldarea, one)
        meanptop = np.where(has, meanptop / safe, miss).astype(R)
        meanalbedocld = np.where(has, meanalbedocld / safe, miss).astype(R)
        alb = np.where(has, meanalbedocld, R(0.5))
        meantaucld = np.where(has, _pow(R(6.82) / ((one / alb) - one), one / R(0.895)), miss).astype(R)
    out = dict(fq_isccp=fq.astype(R), totalcldarea=totalcldarea, meanptop=meanptop, meantaucld=meantaucld, meanalbedocld=meanalbedocld,
               meantb=meantb.astype(R), meantbclr=meantbclr.astype(R), boxtau=boxtau, boxptop=boxptop)
    assert all(v.dtype == R for v in out.values())
    if detail:
        out["itau"], out["ipres"] = itau_all, ipres_all
    return out


def bins_of(boxtau, boxptop):
    """(itau, ipres) of icarus.f:1115-1158 from the two per-sub-column outputs (0 where the sub-column is not binned: missing value)"""
    on = boxptop > 0
    itau = 1 + sum((boxtau >= boxtau.dtype.type(b)).astype(np.int64) for b in (0.3, 1.3, 3.6, 9.4, 23., 60.))
    ipres = 1 + sum((boxptop >= boxptop.dtype.type(b)).astype(np.int64) for b in (180., 310., 440., 560., 680., 800.))
    return np.where(on, itau, 0), np.where(on, ipres, 0)


# ---- cosp.F90:167-174, cosp_isccp_simulator.F90:58-90 ------------------------------------------------------------------------------
def cosp_seeds(psfc, dtype):
    R = np.dtype(dtype).type
    psfc = np.asarray(psfc, dtype=R)
    if psfc.size == 1:
        return np.trunc(psfc).astype(np.int32)
    minp, maxp = psfc.min(), psfc.max()
    return (np.trunc((psfc - minp) / (maxp - minp) * R(100000)).astype(np.int64) + 1).astype(np.int32)


def model_fields(b):
    """The batch as GEOS_SatsimGridComp holds it before it builds gbx (model order = TOA first): PLE (0:LM) whose levels 0..LM-1 are what
    the wrapper hands icarus as phalf(2:), FCLD / CCA before the 0.999999 scaling (the batch's cc / conv are taken as the unscaled fields)"""
    ple = np.concatenate([b["phalf"][1:], (b["phalf"][-1] + (b["phalf"][-1] - b["phalf"][-2]))[None, :]])
    return dict(T=b["at"], QV=b["qv"], FCLD=b["cc"], CCA=b["conv"], PLE=np.ascontiguousarray(ple), PLO=b["pfull"], DTAU_S=b["dtau_s"],
                EMISS=b["dem_s"], DTAU_C=b["dtau_c"], DEM_C=b["dem_c"], TS=b["skt"], sunlit=b["sunlit"], seed=b["seed"])


def cosp_prepare(f, dtype):
    """icarus' arguments as cosp_isccp_simulator.F90:58-72 forms them from model_fields (after the two flips that cancel): phalf(1) = 0,
    phalf(2:) = PLE(0:LM-1), cc / conv scaled by 0.999999.  scops does not get these: cosp.F90:392-397 hands it the fractions as they are"""
    R = np.dtype(dtype).type
    A = lambda x: np.asarray(x, dtype=R)
    ple = A(f["PLE"])
    z = np.zeros_like(A(f["FCLD"]))
    return dict(pfull=A(f["PLO"]), phalf=np.ascontiguousarray(np.concatenate([np.zeros((1, ple.shape[1]), R), ple[:-1]])), qv=A(f["QV"]),
                cc=R(0.999999) * A(f["FCLD"]), conv=R(0.999999) * (A(f["CCA"]) if f.get("CCA") is not None else z), dtau_s=A(f["DTAU_S"]),
                dtau_c=A(f["DTAU_C"]) if f.get("DTAU_C") is not None else z, at=A(f["T"]), dem_s=A(f["EMISS"]),
                dem_c=A(f["DEM_C"]) if f.get("DEM_C") is not None else z, skt=A(f["TS"]))


def cosp_finish(o, dtype):
    """cosp_isccp_simulator.F90:84-90 on icarus' outputs: the pressure flip of fq_isccp and the snap of totalcldarea"""
    R = np.dtype(dtype).type
    o = dict(o)
    o["fq_isccp"] = np.ascontiguousarray(o["fq_isccp"][::-1])
    t = o["totalcldarea"]
    o["totalcldarea"] = np.where((t > R(1.0) - R(1.e-5)) & (t < R(1.0) + R(1.e-5)), R(1.0), t).astype(R)
    return o


def sgfcld(frac_out, dtype):
    """GEOS_SatsimGridComp.F90:3727-3732: the sub-column sum of the mask (a 2 counts as 2) over Ncolumns, (nlev, npoints)"""
    R = np.dtype(dtype).type
    s = np.zeros(frac_out.shape[::2], R)
    for ibox in range(frac_out.shape[1]):
        s = s + frac_out[:, ibox].astype(R)
    return s / (R(1.) * R(frac_out.shape[1]))
