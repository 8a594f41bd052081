"""Helpers of the MISR and MODIS tests: the extra planes of tests/golden/satsim_misr_modis_72.npz (make_hydro) and numpy restatements of
GEOSsatsim_GridComp's MISR_simulator.f and of modis_simulator.F90 with the wrapper rules around it, statement by statement in the real kind it is given - numpy rounds every operation on its own, so
it is un-fused.  The batch itself (96 x 72 x 30), its overlap-3 mask and everything about SCOPS / ICARUS are tests/satsim_util.py's.

Layouts as everywhere in the tests: C order with the point index last, i.e. the reference's Fortran arrays with the point index first:
zfull (nlev, npoints), frac_out (nlev, ncol, npoints), fq_MISR_TAU_v_CTH (16 heights, 7 tau, npoints), dist_model_layertops (16, npoints)."""
import os

import numpy as np

from tests import satsim_util as U

MISSING = U.MISSING          # R_UNDEF, what cosp_misr_simulator.F90:72-74 passes as missing_value
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "satsim_misr_modis_72.npz")
HYDRO = ["zfull", "ql", "qi", "rl", "ri", "qlc", "qic", "rlc", "ric"]
MISR_OUT = ["fq_MISR_TAU_v_CTH", "dist_model_layertops", "MISR_mean_ztop", "MISR_cldarea"]
MISR_CONTINUOUS = ["MISR_mean_ztop", "MISR_cldarea"]
N_CTH = 16
# 1000 * MISR_CTH_boundaries(3:17), MISR_simulator.f:113-114: the lower edges of height bins 3..17 in metres
CTH_EDGES = [500., 1000., 1500., 2000., 2500., 3000., 4000., 5000., 7000., 9000., 11000., 13000., 15000., 17000., 99000.]


def make_hydro(b, seed=20262):
    """Nine planes (nlev, npoints) beside a satsim_util.make_batch() batch, computed in float64 from the batch's float32 values and rounded to
    float32: zfull = 7400 ln(phalf[-1] / pfull); on the stratiform decks (dtau_s > 0) a water content q = 2e-5 exp(3 u) split into liquid and
    ice by fl = clip((at - 243) / 30, 0, 1) with radii U(5e-6, 2.8e-5) and U(8e-6, 8e-5) m; on the convective decks (dtau_c > 0)
    qc = 4e-5 exp(2 u) with radii U(6e-6, 2.6e-5) and U(1e-5, 7e-5) m; zero off the decks.  The radii stay inside the MODIS retrieval's bounds.
    MISR reads zfull only, MODIS the eight others."""
    f = {k: np.asarray(b[k], np.float32).astype(np.float64) for k in ("pfull", "phalf", "at", "dtau_s", "dtau_c")}
    shape = f["pfull"].shape
    deck, cdeck = f["dtau_s"] > 0, f["dtau_c"] > 0
    rng = np.random.default_rng(seed)
    u1, rl, ri, u2, rlc, ric = (rng.uniform(0, 1, shape) for _ in range(6))
    fl = np.clip((f["at"] - 243.0) / 30.0, 0.0, 1.0)
    q = np.where(deck, 2e-5 * np.exp(3.0 * u1), 0.0)
    qc = np.where(cdeck, 4e-5 * np.exp(2.0 * u2), 0.0)
    h = dict(zfull=7400.0 * np.log(f["phalf"][-1][None, :] / f["pfull"]), ql=fl * q, qi=(1.0 - fl) * q,
             rl=np.where(deck, 5e-6 + (2.8e-5 - 5e-6) * rl, 0.0), ri=np.where(deck, 8e-6 + (8e-5 - 8e-6) * ri, 0.0),
             qlc=fl * qc, qic=(1.0 - fl) * qc,
             rlc=np.where(cdeck, 6e-6 + (2.6e-5 - 6e-6) * rlc, 0.0), ric=np.where(cdeck, 1e-5 + (7e-5 - 1e-5) * ric, 0.0))
    return {k: np.ascontiguousarray(h[k].astype(np.float32)) for k in HYDRO}


def roll1(a):
    """the array with its second point first (the point index is the last axis): the fixture's rolled batch"""
    return np.ascontiguousarray(np.roll(a, -1, axis=-1))


def misr_bin(z, R):
    """MISR_simulator.f:139-149, :412-422: the height bin 2..16 (1-based; 1 is "no height") of heights in metres"""
    i = np.full(np.shape(z), 2, np.int64)
    for loop in range(2, N_CTH + 1):
        i = np.where(z > R(CTH_EDGES[loop - 2]), loop + 1, i)
    return i


def misr(sunlit, zfull, at, dtau_s, dtau_c, frac_out, missing_value, dtype, detail=False):
    """MISR_simulator.f for one call: a dict of MISR_OUT (+ with `detail` tau and box_MISR_ztop (ncol, npoints), the latter after the
    pattern matcher).  ncol = 1 (the serial scan over the points of :294-313) is not restated."""
    R = np.dtype(dtype).type
    A = lambda x: np.asarray(x, dtype=R)
    zfull, at, dtau_s, dtau_c = map(A, (zfull, at, dtau_s, dtau_c))
    sunlit = np.asarray(sunlit)
    nlev, npts = zfull.shape
    ncol = frac_out.shape[1]
    if ncol == 1:
        raise ValueError("ncol = 1 couples neighbouring points")
    zero, one, half, miss = R(0), R(1), R(0.5), R(missing_value)
    tauchk = R(-1.) * U._log(R(0.9999999))
    isccp_taumin = R(0.3)
    with np.errstate(all="ignore"):
        # :128-153
        dist = np.zeros((N_CTH, npts), R)
        jj = np.arange(npts)
        for ilev in range(nlev):
            ztest = zfull[ilev] if ilev in (0, nlev - 1) else half * (zfull[ilev] + zfull[ilev - 1])
            i = misr_bin(ztest, R)
            dist[i - 1, jj] = dist[i - 1, jj] + one
        # :159-278
        tau = np.zeros((ncol, npts), R); ztop = np.zeros((ncol, npts), R); cloud_dtau = np.zeros((ncol, npts), R)
        thres = np.zeros((ncol, npts), np.int64)
        for ilev in range(nlev):
            f = frac_out[ilev]
            dtau = np.where(f == 1, dtau_s[ilev][None, :], zero).astype(R)
            dtau = np.where(f == 2, dtau_c[ilev][None, :], dtau).astype(R)
            tau = tau + dtau
            start = (thres == 0) & (dtau > zero)
            thres = np.where(start, 1, thres); cloud_dtau = np.where(start, zero, cloud_dtau)
            act = (thres < 99) & (thres > 0)
            cloud_dtau = np.where(act, np.where(dtau == zero, zero, cloud_dtau + dtau), cloud_dtau).astype(R)
            pen = act & (dtau > zero) & ((cloud_dtau - dtau) < one)
            zk = np.broadcast_to(zfull[ilev][None, :], dtau.shape)
            if ilev in (0, nlev - 1):
                h = zk
            else:
                safe = np.where(dtau > zero, dtau, one)
                deep = half * (zfull[ilev] + zfull[ilev - 1])[None, :] - half * (zfull[ilev - 1] - zfull[ilev + 1])[None, :] / safe
                h = np.where(dtau < one, zk, deep)
            ztop = np.where(pen, h, ztop).astype(R)
            thres = np.where(act & (dtau > one) & (at[ilev][None, :] > R(273)), 99, thres)
            thres = np.where(act & (tau > R(5)), 99, thres)
        open_ = thres == 1      # :254-276
        ztop = np.where(open_ & ~(tau > R(0.5)), np.where(tau > R(0.2), R(-1), zero), ztop).astype(R)
        # :314-335: box_MISR_ztop(1,ibox), the first point of the call, sequentially in ibox
        for ibox in range(1, ncol - 1):
            a, c = ztop[ibox - 1, 0], ztop[ibox + 1, 0]
            if a > zero and c > zero and abs(a - c) < R(500) and ztop[ibox, 0] < c:
                ztop[ibox, 0] = c
        # :342-470
        lit = sunlit == 1
        boxarea = R(1.) / R(ncol)
        fq = np.zeros((N_CTH, 7, npts), R); cldarea = np.zeros(npts, R); mean_ztop = np.zeros(npts, R)
        taub = [1.3, 3.6, 9.4, 23., 60.]
        for ibox in range(ncol):
            t, z = tau[ibox], ztop[ibox]
            cloudy = t > tauchk
            itau = np.where(cloudy, np.where(t < isccp_taumin, 1, 2 + sum((t >= R(b)).astype(np.int64) for b in taub)), 0)
            thin = lit & (z == R(-1))
            high = lit & (z != zero) & (z != R(-1))
            iz = np.where(thin, 1, misr_bin(z, R))
            hit = (thin | (high & cloudy)) & (itau >= 1)
            fq[iz[hit] - 1, itau[hit] - 1, jj[hit]] = fq[iz[hit] - 1, itau[hit] - 1, jj[hit]] + boxarea
            mean_ztop = np.where(high, mean_ztop + z * boxarea, mean_ztop).astype(R)
            cldarea = np.where(high, cldarea + boxarea, cldarea).astype(R)
        # :451-462: a dark point; the statement for the mean height sets MISR_mean_ztop(npoints), which that point resets at its own turn
        fq[:, :, ~lit] = miss; dist[:, ~lit] = miss; cldarea[~lit] = miss
        if not lit[-1]:
            mean_ztop[-1] = miss
        pos = cldarea > zero      # :466-468
        mean_ztop = np.where(pos, mean_ztop / np.where(pos, cldarea, one), mean_ztop).astype(R)
    out = dict(fq_MISR_TAU_v_CTH=fq, dist_model_layertops=dist, MISR_mean_ztop=mean_ztop, MISR_cldarea=cldarea)
    assert all(v.dtype == R for v in out.values())
    if detail:
        out["tau"], out["ztop"] = tau, ztop
    return out


def misr_counts(fq, ncol, missing_value=MISSING):
    """the histogram as whole sub-columns per cell (0 where the point is dark): fq is a sum of `count` additions of 1 / ncol"""
    f = np.asarray(fq, np.float64)
    return np.where(f == np.float64(np.asarray(fq).dtype.type(missing_value)), 0, np.rint(f * ncol)).astype(np.int64)


# ---- modis_simulator.F90 and the rules of cosp.F90 / cosp_modis_simulator.F90 around it -----------------------------------------------------
R_UNDEF = -1.0e30
MODIS_MEAN = ["cf_total", "cf_water", "cf_ice", "cf_high", "cf_mid", "cf_low", "tau_total", "tau_water", "tau_ice", "logtau_total", "logtau_water",
              "logtau_ice", "size_water", "size_ice", "ctp_total", "lwp", "iwp"]          # modis_L3_simulator's argument order, :386-392
MODIS_L2 = ["phase", "ctp", "tau", "size"]
N_TRIAL = 15


def _sqrt(x):
    return np.sqrt(x)


def _log10(x):
    return np.log10(np.asarray(x, np.float64)).astype(np.asarray(x).dtype)


def modis_range_check(sunlit, t, p, dtau_s, dtau_c, frac_out, reff_lsliq, reff_lsice, reff_cvliq, reff_cvice):
    """modis_simulator.F90:202-206 on what the wrapper hands it (sunlit points only, a cell's stratiform / convective values only where a
    sub-column of the cell is stratiform / convective): the names of the offending arrays, in the order the library reports them"""
    lit = (np.asarray(sunlit) > 0)[None, :]
    ls, cv = (frac_out == 1).any(axis=1), (frac_out == 2).any(axis=1)
    z = np.zeros_like(t)
    Z = lambda a: z if a is None else a
    checks = [("t", (t <= 0)), ("p", (p <= 0)), ("dtau_s", (dtau_s < 0) & ls), ("dtau_c", (Z(dtau_c) < 0) & cv), ("reff_lsliq", (reff_lsliq < 0) & ls),
              ("reff_lsice", (reff_lsice < 0) & ls), ("reff_cvliq", (Z(reff_cvliq) < 0) & cv), ("reff_cvice", (Z(reff_cvice) < 0) & cv)]
    return [n for n, bad in checks if (bad & lit).any()]


def modis_subcolumns(dtau_s, dtau_c, frac_out, mr_lsliq, mr_lsice, mr_cvliq, mr_cvice, reff_lsliq, reff_lsice, reff_cvliq, reff_cvice, dtype):
    """cosp.F90:414-431, :453-470, :484-494 and cosp_modis_simulator.F90:146-170: a sub-column's optical thickness, water and ice content and
    the two radii per cell, (nlev, ncol, npoints) each.  None for a convective array: zero"""
    R = np.dtype(dtype).type
    ncol = frac_out.shape[1]
    z = np.zeros(np.shape(dtau_s), R)
    A = lambda x: z if x is None else np.asarray(x, dtype=R)
    ls, cv = frac_out == 1, frac_out == 2
    with np.errstate(all="ignore"):
        frac_ls = (ls.sum(axis=1).astype(R) / R(ncol))[:, None, :]
        frac_cv = (cv.sum(axis=1).astype(R) / R(ncol))[:, None, :]
        B = lambda x: A(x)[:, None, :]
        pick = lambda a, c: np.where(ls, a, np.where(cv, c, R(0))).astype(R)
        return (pick(B(dtau_s), B(dtau_c)), pick(B(mr_lsliq) / frac_ls, B(mr_cvliq) / frac_cv), pick(B(mr_lsice) / frac_ls, B(mr_cvice) / frac_cv),
                pick(B(reff_lsliq), B(reff_cvliq)), pick(B(reff_lsice), B(reff_cvice)))


def _quad(x, c, R):
    return R(c[0]) + x * (R(c[1]) + x * (R(c[2])))


def _cubic(x, c, R):
    return R(c[0]) + x * (R(c[1]) + x * (R(c[2]) + x * R(c[3])))


def modis_g_nir(liquid, re, R):
    """get_g_nir, :726-756"""
    re = np.asarray(re, R)
    if liquid:
        small = _quad(np.maximum(re, R(4.)), (0.8027, -1.0496e-2, 1.7071e-3), R)
        big = _quad(np.minimum(re, R(30.)), (0.7931, 5.3087e-3, -7.4995e-5), R)
        return np.where(re < R(8.), small, big).astype(R)
    return _quad(np.minimum(np.maximum(re, R(5.)), R(90.)), (0.7432, 4.5563e-3, -2.8697e-5), R).astype(R)


def modis_ssa_nir(liquid, re, R):
    """get_ssa_nir, :759-783"""
    re = np.asarray(re, R)
    if liquid:
        return _quad(np.minimum(np.maximum(re, R(4.)), R(30.)), (1.0008, -2.5626e-3, 1.6024e-5), R).astype(R)
    return _cubic(np.minimum(np.maximum(re, R(5.)), R(90.)), (0.9994, -4.5199e-3, 3.9370e-5, -1.5235e-7), R).astype(R)


def modis_two_stream(tauint, gint, w0int, R):
    """two_stream / two_stream_reflectance with beam = 2, :830-982: (reflectance, transmittance)"""
    one = R(1)
    f = gint * gint
    tau = (one - w0int * f) * tauint
    w0 = (one - f) * w0int / (one - w0int * f)
    g = (gint - f) / (one - f)
    gamma1 = (R(7) - w0 * (R(4) + R(3) * g)) / R(4.0)
    gamma2 = -(one - w0 * (R(4) - R(3) * g)) / R(4.0)
    xmu = R(0.866)
    cons_ref = gamma1 * tau / (one + gamma1 * tau)
    rk = _sqrt(gamma1 * gamma1 - gamma2 * gamma2)
    r4 = (one - (rk * xmu) * (rk * xmu)) * (rk + gamma1)
    r5 = (one - (rk * xmu) * (rk * xmu)) * (rk - gamma1)
    beta = -r5 / r4
    e1 = np.minimum(rk * tau, R(500.))
    ef1 = U._exp(-e1)
    ef2 = U._exp(R(-2) * e1)
    ref = (gamma2 * (one - ef2)) / ((rk + gamma1) * (one - beta * ef2))
    tra = (R(2) * rk * ef1) / ((rk + gamma1) * (one - beta * ef2))
    cons = w0int > R(0.9999999)
    return np.where(cons, cons_ref, ref).astype(R), np.where(cons, one - cons_ref, tra).astype(R)


def modis_trial_tables(R):
    """trial_re_w, trial_re_i (:85-87) and the g, w0 of :235-238 in the real kind"""
    i = np.arange(N_TRIAL).astype(R)
    tw = R(4.) + (R(30.) - R(4.)) / R(N_TRIAL - 1) * i
    ti = R(5.) + (R(90.) - R(5.)) / R(N_TRIAL - 1) * i
    return dict(re_w=tw.astype(R), g_w=modis_g_nir(True, tw, R), w0_w=modis_ssa_nir(True, tw, R),
                re_i=ti.astype(R), g_i=modis_g_nir(False, ti, R), w0_i=modis_ssa_nir(False, ti, R))


def modis_l2(t, p, ph, tau_c, water, ice, rw, ri, isccp_boxptop, dtype):
    """modis_L2_simulator_oneTau + _twoTaus for every point at once: cell arrays (nlev, ncol, npoints), ph (nlev + 1, npoints), boxptop
    (ncol, npoints) in hPa.  Returns phase (int32), ctp, tau, size, (ncol, npoints)"""
    R = np.dtype(dtype).type
    A = lambda x: np.asarray(x, dtype=R)
    ph, tau_c, water, ice, rw, ri, boxptop = map(A, (ph, tau_c, water, ice, rw, ri, isccp_boxptop))
    nlev, ncol, npts = tau_c.shape
    one, zero, undef = R(1), R(0), R(R_UNDEF)
    with np.errstate(all="ignore"):
        share = np.where(ice <= zero, one, np.where(water <= zero, zero, (water / rw) / (water / rw + ice / (R(0.93) * ri)))).astype(R)
        tl = share * tau_c
        ti = tau_c - tl
        tt = tl + ti
        lf = np.where(tt > zero, tl / tt, zero).astype(R)
        total = np.zeros((ncol, npts), R)
        for k in range(nlev):
            total = total + tt[k]
        cloudy = total >= R(0.3)
        # cloud_top_pressure (:531-562) and weight_by_extinction (:564-588), limit 1
        ctau = np.zeros((ncol, npts), R); cprod = np.zeros((ncol, npts), R); cdone = np.zeros((ncol, npts), bool)
        wtau = np.zeros((ncol, npts), R); wprod = np.zeros((ncol, npts), R); wdone = np.zeros((ncol, npts), bool)
        lim = one
        for k in range(nlev):
            inc = tt[k]
            p0, p1 = ph[k][None, :], ph[k + 1][None, :]
            part = (ctau + inc > lim)
            dx = lim - ctau
            safe = np.where(inc != zero, inc, one)
            ntau = np.where(part, ctau + dx, ctau + inc)
            nprod = np.where(part, cprod + p0 * dx + (p1 - p0) * (dx * dx) / (R(2.) * safe), cprod + inc * (p1 + p0) / R(2.))
            ctau = np.where(cdone, ctau, ntau).astype(R); cprod = np.where(cdone, cprod, nprod).astype(R)
            cdone = cdone | (ctau >= lim)
            part = (wtau + inc > lim)
            dx = lim - wtau
            ntau = np.where(part, wtau + dx, wtau + inc)
            nprod = np.where(part, wprod + dx * lf[k], wprod + inc * lf[k])
            wtau = np.where(wdone, wtau, ntau).astype(R); wprod = np.where(wdone, wprod, nprod).astype(R)
            wdone = wdone | (wtau >= lim)
        ctp = cprod / ctau
        ilf = wprod / wtau
        phase = np.where(ilf >= R(0.7), 1, np.where(ilf <= one - R(0.7), 2, 3))
        # compute_nir_reflectance (:590-614) with compute_toa_reflectace (:805-828): only the layers with tau > 0, added from the top
        rc = np.zeros((ncol, npts), R); tc = np.zeros((ncol, npts), R); first = np.ones((ncol, npts), bool)
        for k in range(nlev):
            rwu, riu = rw[k] * R(1.0e6), ri[k] * R(1.0e6)
            wg, ww0, ig, iw0 = modis_g_nir(True, rwu, R), modis_ssa_nir(True, rwu, R), modis_g_nir(False, riu, R), modis_ssa_nir(False, riu, R)
            tau = ti[k] + tl[k]
            on = tau > zero
            st = np.where(on, tau, one)
            g = (tl[k] * wg + ti[k] * ig) / st
            w0 = (tl[k] * wg * ww0 + ti[k] * ig * iw0) / (g * st)
            ref, tra = modis_two_stream(st, g, w0, R)
            nr = rc + ref * (tc * tc) / (one - rc * ref)
            nt = (tc * tra) / (one - rc * ref)
            rc2 = np.where(first, ref, nr); tc2 = np.where(first, tra, nt)
            rc = np.where(on, rc2, rc).astype(R); tc = np.where(on, tc2, tc).astype(R)
            first = first & ~on
        obs = rc
        # retrieve_re (:618-678) with interpolate_to_min (:680-722)
        T = modis_trial_tables(R)
        liq = (phase == 1) | (phase == 3)
        diffs, xs = [], []
        for i in range(N_TRIAL):
            g = np.where(liq, T["g_w"][i], T["g_i"][i]).astype(R); w0 = np.where(liq, T["w0_w"][i], T["w0_i"][i]).astype(R)
            pred, _ = modis_two_stream(total, g, w0, R)
            diffs.append(pred - obs); xs.append(np.where(liq, T["re_w"][i], T["re_i"][i]).astype(R))
        diff, x = np.stack(diffs), np.stack(xs)
        m = np.argmin(np.abs(diff), axis=0)          # the first minimum, as minloc
        take = lambda a, i: np.take_along_axis(a, np.clip(i, 0, N_TRIAL - 1)[None], axis=0)[0]
        inner_low = take(diff, m - 1) * take(diff, m) < zero
        lb = np.where(m == 0, 0, np.where(m == N_TRIAL - 1, N_TRIAL - 2, np.where(inner_low, m - 1, m)))
        ub = lb + 1
        dl, du, xl, xu = take(diff, lb), take(diff, ub), take(x, lb), take(x, ub)
        re = np.where(dl * du < zero, xu - du * (xu - xl) / (du - dl), R(-999.)).astype(R)
        size = R(1.0e-06) * re
        size = np.where((size < zero) & (size != undef), R(1.0e-06) * R(-999.), size)
        ctp = np.where(cloudy & (ctp > R(700.) * R(100.)), boxptop * R(100.), ctp)
    return (np.where(cloudy, phase, 0).astype(np.int32), np.where(cloudy, ctp, undef).astype(R), np.where(cloudy, total, undef).astype(R),
            np.where(cloudy, size, undef).astype(R))


def modis_l3(phase, ctp, tau, size, dtype):
    """modis_L3_simulator (:445-527) on (ncol, npoints) arrays: the 17 means (17, npoints) in MODIS_MEAN's order and the joint histogram
    (7 pressure bins, 6 tau bins, npoints), pressure from the top down as the routine leaves it"""
    R = np.dtype(dtype).type
    ncol, npts = phase.shape
    one, zero = R(1), R(0)
    with np.errstate(all="ignore"):
        valid = size > zero
        cm, wm, im = (phase != 0) & valid, (phase == 1) & valid, (phase == 2) & valid

        def msum(a, m):
            s = np.zeros(npts, R)
            for b in range(ncol):
                s = np.where(m[b], s + a[b], s).astype(R)
            return s
        cnt = lambda m: m.sum(axis=0).astype(R)
        cT, cW, cI = cnt(cm), cnt(wm), cnt(im)
        hi, lo = cnt(cm & (ctp <= R(440.) * R(100.))), cnt(cm & (ctp > R(680.) * R(100.)))
        mid = cT - hi - lo
        nT, nW, nI = (np.where(c == zero, R(-1.), c).astype(R) for c in (cT, cW, cI))
        lt = _log10(np.abs(tau))
        conv = R(2.) / R(3.) * R(1000.)
        mean = [None] * 17
        mean[6], mean[7], mean[8] = msum(tau, cm) / nT, msum(tau, wm) / nW, msum(tau, im) / nI
        mean[9], mean[10], mean[11] = msum(lt, cm) / nT, msum(lt, wm) / nW, msum(lt, im) / nI
        mean[12], mean[13] = msum(size, wm) / nW, msum(size, im) / nI
        mean[14] = msum(ctp, cm) / np.maximum(1, cm.sum(axis=0)).astype(R)
        mean[15] = conv * msum(size * tau, wm) / nW
        mean[16] = conv * R(0.93) * msum(size * tau, im) / nI
        mean[0], mean[1], mean[2] = (np.maximum(zero, c / R(ncol)) for c in (nT, nW, nI))
        mean[3], mean[4], mean[5] = hi / R(ncol), mid / R(ncol), lo / R(ncol)
        tb = [R(0.3), R(1.3), R(3.6), R(9.4), R(23.), R(60.), np.finfo(R).max]
        pb = [R(0.), R(18000.), R(31000.), R(44000.), R(56000.), R(68000.), R(80000.), np.finfo(R).max]
        hist = np.zeros((7, 6, npts), R)
        for ip in range(7):
            for it in range(6):
                hit = cm & (tau >= tb[it]) & (tau < tb[it + 1]) & (ctp >= pb[ip]) & (ctp < pb[ip + 1])
                hist[ip, it] = hit.sum(axis=0).astype(R) / R(ncol)
    return np.stack([np.asarray(m, R) for m in mean]).astype(R), hist


def modis_wrap(sunlit, mean, hist, l2, dtype):
    """cosp_modis_simulator.F90:124-294 around the L2 / L3 results of every point: a dark point (sunlit <= 0) gets R_UNDEF everywhere and
    phase 0; the histogram becomes (7 pressure, 7 tau, npoints) with tau index 1 left R_UNDEF (:338-339, :229) and the pressure reversed
    (:233-234)"""
    R = np.dtype(dtype).type
    dark = ~(np.asarray(sunlit) > 0)
    undef = R(R_UNDEF)
    mean = np.where(dark[None, :], undef, mean).astype(R)
    h = np.full((7, 7, hist.shape[-1]), undef, R)
    h[:, 1:, :] = hist[::-1]
    h[:, :, dark] = undef
    phase, ctp, tau, size = l2
    return mean, h, (np.where(dark[None, :], 0, phase).astype(np.int32),) + tuple(np.where(dark[None, :], undef, a).astype(R) for a in (ctp, tau, size))


def modis(sunlit, t, p, ph, dtau_s, dtau_c, frac_out, mr_lsliq, mr_lsice, mr_cvliq, mr_cvice, reff_lsliq, reff_lsice, reff_cvliq, reff_cvice,
          isccp_boxptop, dtype):
    """geosrad_modis as a whole: dict(modis_mean (17, npoints), modis_hist (7, 7, npoints), phase, ctp, tau, size (ncol, npoints));
    ValueError naming the array where modis_simulator.F90:202-206 stops"""
    R = np.dtype(dtype).type
    bad = modis_range_check(sunlit, np.asarray(t, R), np.asarray(p, R), np.asarray(dtau_s, R), None if dtau_c is None else np.asarray(dtau_c, R), frac_out,
                            np.asarray(reff_lsliq, R), np.asarray(reff_lsice, R), None if reff_cvliq is None else np.asarray(reff_cvliq, R),
                            None if reff_cvice is None else np.asarray(reff_cvice, R))
    if bad:
        raise ValueError("Input values out of bounds: " + bad[0])
    cells = modis_subcolumns(dtau_s, dtau_c, frac_out, mr_lsliq, mr_lsice, mr_cvliq, mr_cvice, reff_lsliq, reff_lsice, reff_cvliq, reff_cvice, dtype)
    l2 = modis_l2(t, p, ph, *cells, isccp_boxptop, dtype)
    mean, hist = modis_l3(*l2, dtype)
    mean, hist, l2 = modis_wrap(sunlit, mean, hist, l2, dtype)
    return dict(modis_mean=mean, modis_hist=hist, phase=l2[0], ctp=l2[1], tau=l2[2], size=l2[3])
