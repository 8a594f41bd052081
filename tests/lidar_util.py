"""Helpers of the lidar tests: the extra inputs of tests/golden/satsim_lidar_72.npz (make_lidar_inputs) and a numpy restatement of
GEOSsatsim_GridComp's COSP_LIDAR (cosp_lidar.F90:44-82) with lidar_simulator and parasol (actsim/lidar_simulator.F90) and of diag_lidar
with COSP_CLDFRAC and COSP_CFAD_SR (actsim/lmd_ipsl_stats.F90) as cosp_stats.F90:126-140 calls it and leaves its results, statement by
statement in the real kind it is given, in the reference's operation order - numpy rounds every operation on its own, so it is un-fused.
The batch itself (96 x 72 x 30) and its overlap-3 mask are tests/satsim_util.py's, its water contents and radii
tests/satsim_misr_modis_util.make_hydro's.

Layouts as everywhere in the tests: C order with the point index last, i.e. the reference's Fortran arrays with the point index first, and
the top of the atmosphere first (the reference counts from the surface: its level k is level nlev+1-k here): p (nlev, npoints), presf
(nlev + 1, npoints), frac_out (nlev, ncol, npoints), cfad_sr (nlev, 15, npoints), cldlayer (4, npoints), parasolrefl (5, npoints), refl (5,
ncol, npoints)."""
import os

import numpy as np

from tests import satsim_util as U

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "satsim_lidar_72.npz")
R_UNDEF = -1.0e30
LIDAR_UNDEF = 999.999
NBIN, NREFL, NCAT = 15, 5, 4
STATS = ["lidarcld", "cldlayer", "cfad_sr", "parasolrefl"]
LIDAR_OUT = STATS + ["pmol", "beta_tot", "tau_tot", "refl"]
CONTINUOUS = ["lidarcld", "cldlayer", "parasolrefl", "pmol", "beta_tot", "tau_tot", "refl"]
GRID = ["p", "t", "pplay", "mr_lsliq", "mr_lsice", "mr_cvliq", "mr_cvice", "reff_lsliq", "reff_lsice", "reff_cvliq", "reff_cvice"]
ABOVE, NOBIN, UNDEF_CODE = 15, 16, 255          # bin codes beside 0..14: above the last edge, in no bin, undefined

# polpart, lidar_simulator.F90:200-241: liquid; ice for ice_type 0 and 1
POL_LIQ = (2.6980e-8, -3.7701e-6, 1.6594e-4, -0.0024, 0.0626)
POL_ICE = ((-1.0176e-8, 1.7615e-6, -1.0480e-4, 0.0019, 0.0460), (1.3615e-8, -2.04206e-6, 7.51799e-5, 0.00078213, 0.0182131))
# parasol's look-up tables, :465-490
TAU = (0., 1., 5., 10., 20., 50., 100.)
TETAS = (0., 20., 40., 60., 80.)
RLUM_A = ((0.03, 0.090886, 0.283965, 0.480587, 0.695235, 0.908229, 1.0), (0.03, 0.072185, 0.252596, 0.436401, 0.631352, 0.823924, 0.909013),
          (0.03, 0.058410, 0.224707, 0.367451, 0.509180, 0.648152, 0.709554), (0.03, 0.052498, 0.175844, 0.252916, 0.326551, 0.398581, 0.430405),
          (0.03, 0.034730, 0.064488, 0.081667, 0.098215, 0.114411, 0.121567))
RLUM_B = ((0.03, 0.092170, 0.311941, 0.511298, 0.712079, 0.898243, 0.976646), (0.03, 0.087082, 0.304293, 0.490879, 0.673565, 0.842026, 0.912966),
          (0.03, 0.083325, 0.285193, 0.430266, 0.563747, 0.685773, 0.737154), (0.03, 0.084935, 0.233450, 0.312280, 0.382376, 0.446371, 0.473317),
          (0.03, 0.054157, 0.089911, 0.107854, 0.124127, 0.139004, 0.145269))


def make_lidar_inputs(b):
    """What the lidar needs beside a satsim_util.make_batch() batch and make_hydro(): p = the batch's pfull and presf = its phalf (the true
    layer edges, 0 at the top), both scaled by 0.04 on every sixth point - a column whose layers are a few hPa thin, where a cloud's
    scattering ratio passes the last bin edge (the ratio of a layer is bounded by about 3.2e5 / its thickness in Pa); pplay = presf without
    its last level, the upper edge of each layer, which is what GEOS hands COSP_CLDFRAC (its top value, 0, fails `p1 > 0` and falls into
    the low category as in the reference); land = 1 on every third point, else 0."""
    j = np.arange(b["phalf"].shape[1])
    scale = np.where(j % 6 == 4, np.float32(0.04), np.float32(1.0))[None, :]
    presf = (np.asarray(b["phalf"], np.float32) * scale).astype(np.float32)
    return dict(p=(np.asarray(b["pfull"], np.float32) * scale).astype(np.float32), presf=np.ascontiguousarray(presf),
                pplay=np.ascontiguousarray(presf[:-1]), land=(j % 3 == 1).astype(np.float32))


def thicken(hy, b, factor=40.0, every=5):
    """make_hydro()'s contents with those of every fifth point multiplied by `factor`: decks that attenuate the beam fully, so that levels
    below them have no usable sub-column"""
    j = (np.arange(b["phalf"].shape[1]) % every == 2)[None, :]
    out = dict(hy)
    for k in ("ql", "qi", "qlc", "qic"):
        out[k] = np.where(j, hy[k] * np.float32(factor), hy[k]).astype(np.float32)
    return out


def srbval(R):
    """COSP_CFAD_SR's bin edges, lmd_ipsl_stats.F90:223-236, with xmax = undef - 1.0 of :113"""
    e = [R(0.01), R(1.2), R(3.0), R(5.0), R(7.0), R(10.0)]
    for _ in range(7, 11):
        e.append(e[-1] + R(5.0))
    for _ in range(11, 14):
        e.append(e[-1] + R(10.0))
    e.append(R(80.0))
    e.append(R(LIDAR_UNDEF) - R(1.0))
    return e


def subcolumns(frac_out, mr_lsliq, mr_lsice, mr_cvliq, mr_cvice, dtype):
    """cosp.F90:414-431, :453-470, :484-494: the four in-cloud contents of every sub-column's cells, (nlev, ncol, npoints) each.  A stratiform
    cell carries the ls contents over the cell's stratiform fraction, a convective one the cv contents over the convective fraction, every
    other entry is zero.  None for a convective array: zero"""
    R = np.dtype(dtype).type
    ncol = frac_out.shape[1]
    z = np.zeros(np.shape(mr_lsliq), R)
    B = lambda x: (z if x is None else np.asarray(x, dtype=R))[:, None, :]
    ls, cv = frac_out == 1, frac_out == 2
    with np.errstate(all="ignore"):
        frac_ls = (ls.sum(axis=1).astype(R) / R(ncol))[:, None, :]
        frac_cv = (cv.sum(axis=1).astype(R) / R(ncol))[:, None, :]
        return (np.where(ls, B(mr_lsliq) / frac_ls, R(0)).astype(R), np.where(ls, B(mr_lsice) / frac_ls, R(0)).astype(R),
                np.where(cv, B(mr_cvliq) / frac_cv, R(0)).astype(R), np.where(cv, B(mr_cvice) / frac_cv, R(0)).astype(R))


def _cos(x):
    return np.cos(np.asarray(x, np.float64)).astype(np.asarray(x).dtype)


def parasol(sl, si, dtype):
    """parasol, lidar_simulator.F90:505-550, on tautot_S_liq / tautot_S_ice of any shape: refl (5, ...)"""
    R = np.dtype(dtype).type
    tau = [R(x) for x in TAU]
    zero = R(0)
    with np.errstate(all="ignore"):
        pi = np.arccos(np.float64(-1.0)).astype(R) if R is np.float64 else R(np.float32(np.arccos(np.float64(-1.0))))
        sl = np.maximum(sl, tau[0]); si = np.maximum(si, tau[0])
        ts = si + sl
        pos = ts > zero
        safe = np.where(pos, ts, R(1))
        fl = np.where(pos, sl / safe, R(1.)).astype(R); fi = np.where(pos, si / safe, R(0.)).astype(R)
        ts = np.minimum(ts, tau[-1])
        out = []
        for it in range(NREFL):
            r_norm = R(1.) / _cos(pi / R(180.) * R(TETAS[it]))
            ra = np.zeros(np.shape(ts), R); rb = np.zeros(np.shape(ts), R)
            for ny in range(len(TAU) - 1):
                aA = (R(RLUM_A[it][ny + 1]) - R(RLUM_A[it][ny])) / (tau[ny + 1] - tau[ny])
                bA = R(RLUM_A[it][ny]) - aA * tau[ny]
                aB = (R(RLUM_B[it][ny + 1]) - R(RLUM_B[it][ny])) / (tau[ny + 1] - tau[ny])
                bB = R(RLUM_B[it][ny]) - aB * tau[ny]
                hit = (ts >= tau[ny]) & (ts <= tau[ny + 1])
                ra = np.where(hit, aA * ts + bA, ra).astype(R); rb = np.where(hit, aB * ts + bB, rb).astype(R)
            out.append(((fl * ra + fi * rb) * r_norm).astype(R))
    return np.stack(out)


def simulate(p, t, presf, cells, reff, ice_type, dtype):
    """lidar_simulator (lidar_simulator.F90:245-407) for every sub-column at once.  p, t (nlev, npoints), presf (nlev + 1, npoints); cells =
    the four contents (nlev, ncol, npoints) of subcolumns(); reff = the four gridbox radii (nlev, npoints), None = zero.  Returns pmol
    (nlev, npoints), pnorm, tautot (nlev, ncol, npoints), refl (5, ncol, npoints)"""
    R = np.dtype(dtype).type
    A = lambda x: np.asarray(x, dtype=R)
    p, t, presf = A(p), A(t), A(presf)
    nlev, npts = p.shape
    ncol = cells[0].shape[1]
    zero, one = R(0), R(1)
    rhopart = [R(1.0e+03), R(0.5e+03), R(1.0e+03), R(0.5e+03)]
    pol = [POL_LIQ, POL_ICE[ice_type], POL_LIQ, POL_ICE[ice_type]]
    with np.errstate(all="ignore"):
        pi = R(np.arccos(np.float64(-1.0)))
        rhoair = p / (R(287.04) * t)
        rad = [np.minimum(np.maximum(np.zeros((nlev, npts), R) if r is None else A(r), R(0.)), R(70.0e-6)) for r in reff]
        # :262-266: the heights from the surface up; level nlev (here) is the reference's level 1
        z = np.zeros((nlev + 1, npts), R)
        for k in range(nlev - 1, -1, -1):
            z[k] = z[k + 1] - (presf[k] - presf[k + 1]) / (rhoair[k] * R(9.81))
        dz = z[:-1] - z[1:]
        beta_mol = p / R(1.38e-23) / t * R(6.2446e-32)
        alpha_mol = R(8.0) * pi / R(3.0) * beta_mol
        kp = []
        for i in range(4):
            x = rad[i] * R(1e6)
            x2 = x * x
            c = [R(v) for v in pol[i]]
            kp.append(np.where(rad[i] > zero, c[0] * (x2 * x2) + c[1] * (x2 * x) + c[2] * x2 + c[3] * x + c[4], zero).astype(R))
        alpha = []
        for i in range(4):
            ok = (rad[i] > zero)[:, None, :]
            den = np.where(rad[i] > zero, rhopart[i] * rad[i], one)[:, None, :]
            alpha.append(np.where(ok, R(3.0) / R(4.0) * R(2.0) * rhoair[:, None, :] * cells[i] / den, zero).astype(R))
        # :320-338: the optical depths as running sums from the top
        tau_mol = alpha_mol * dz
        for k in range(1, nlev):
            tau_mol[k] = tau_mol[k] + tau_mol[k - 1]
        tau_part = []
        for i in range(4):
            tp = R(0.7) * alpha[i]
            tp = tp * dz[:, None, :]
            for k in range(1, nlev):
                tp[k] = tp[k] + tp[k - 1]
            tau_part.append(tp)

        def signal(beta, tau):
            out = np.empty_like(tau)
            out[0] = beta[0] / (R(2.) * tau[0]) * (one - U._exp(R(-2.0) * tau[0]))
            for k in range(1, nlev):
                lay = tau[k] - tau[k - 1]
                safe = np.where(lay > zero, lay, one)
                a = beta[k] * U._exp(R(-2.0) * tau[k - 1]) / (R(2.) * safe) * (one - U._exp(R(-2.0) * safe))
                out[k] = np.where(lay > zero, a, beta[k] * U._exp(R(-2.0) * tau[k - 1]))
            return out.astype(R)
        pmol = signal(beta_mol, tau_mol)
        betatot = np.broadcast_to(beta_mol[:, None, :], (nlev, ncol, npts)).astype(R)
        tautot = np.broadcast_to(tau_mol[:, None, :], (nlev, ncol, npts)).astype(R)
        for i in range(4):
            betatot = betatot + kp[i][:, None, :] * alpha[i]
            tautot = tautot + tau_part[i]
        pnorm = signal(betatot, tautot)
        sl = zero + tau_part[0][-1] + tau_part[2][-1]
        si = zero + tau_part[1][-1] + tau_part[3][-1]
        refl = parasol(sl, si, dtype)
    assert pmol.dtype == R and pnorm.dtype == R and tautot.dtype == R and refl.dtype == R
    return pmol, pnorm, tautot, refl


def bin_codes(pnorm, pmol, dtype):
    """the scattering ratio of lmd_ipsl_stats.F90:125-133 as its CFAD bin (:245-251): 0..14, ABOVE for a ratio above the last edge, NOBIN for
    one at or below -1, UNDEF_CODE where it is undefined; and the ratio itself (LIDAR_UNDEF where undefined)"""
    R = np.dtype(dtype).type
    undef = R(LIDAR_UNDEF)
    xmax = undef - R(1.0)
    pm = pmol[:, None, :]
    with np.errstate(all="ignore"):
        ok = (pnorm < xmax) & (pm < xmax) & (pm > R(0.0))
        x = np.where(ok, pnorm / np.where(pm > R(0), pm, R(1)), undef).astype(R)
        code = np.zeros(x.shape, np.int64)
        for e in srbval(R):
            code += x > e
        code = np.where(x > R(-1.0), code, NOBIN)
    return np.where(ok, code, UNDEF_CODE).astype(np.uint8), x


def stats(code, refl, land, pplay, dtype):
    """diag_lidar's results from the bin codes (S_cld = 5 and S_att = 0.01 are bin edges: cloudy = codes 4..ABOVE, usable = 1..ABOVE), with
    cosp_stats.F90:137-140: lidarcld (nlev, npoints), cldlayer (4, npoints), cfad_sr (nlev, 15, npoints), parasolrefl (5, npoints)"""
    R = np.dtype(dtype).type
    nlev, ncol, npts = code.shape
    undef, lundef = R(R_UNDEF), R(LIDAR_UNDEF)
    pplay, land = np.asarray(pplay, R), np.asarray(land, R)
    cloudy = (code >= 4) & (code <= ABOVE)
    usable = (code >= 1) & (code <= ABOVE)
    with np.errstate(all="ignore"):
        nc, ns = cloudy.sum(axis=1).astype(R), usable.sum(axis=1).astype(R)
        lidarcld = np.where(ns > R(0), nc / np.where(ns > R(0), ns, R(1)), undef).astype(R)
        high = (pplay > R(0.)) & (pplay < R(440.) * R(100.))
        mid = ~high & (pplay >= R(440.) * R(100.)) & (pplay < R(680.) * R(100.))
        low = ~high & ~mid
        cldlayer = np.empty((NCAT, npts), R)
        for iz, m in enumerate((low, mid, high, np.ones_like(low))):
            c = (cloudy & m[:, None, :]).any(axis=0).sum(axis=0).astype(R)
            s = (usable & m[:, None, :]).any(axis=0).sum(axis=0).astype(R)
            cldlayer[iz] = np.where(s > R(0), c / np.where(s > R(0), s, R(1)), undef)
        off = (code == UNDEF_CODE).any(axis=1)
        cfad = np.stack([np.where(off, undef, (code == b).sum(axis=1).astype(R) / R(ncol)) for b in range(NBIN)], axis=1).astype(R)
        par = np.zeros((NREFL, npts), R)
        for ic in range(ncol):
            par = par + refl[:, ic]
        par = par / R(ncol)
        m = np.maximum(R(1.0) - land, R(0.0))[None, :]
        par = par * m + (R(1.0) - m) * lundef
        par = np.where(par == lundef, undef, par).astype(R)
    return dict(lidarcld=lidarcld, cldlayer=cldlayer, cfad_sr=cfad, parasolrefl=par)


def range_check(p, t):
    """the names of the arrays with a value <= 0, in the order the library reports them"""
    return [n for n, a in (("p", p), ("t", t)) if (np.asarray(a) <= 0).any()]


def lidar(ice_type, p, t, presf, pplay, frac_out, mr_lsliq, mr_lsice, mr_cvliq, mr_cvice, reff_lsliq, reff_lsice, reff_cvliq, reff_cvice, land,
          dtype):
    """geosrad_lidar as a whole: a dict of LIDAR_OUT plus `code`, the bin codes (nlev, ncol, npoints); ValueError naming the array where the
    library reports an input out of bounds"""
    bad = range_check(p, t)
    if bad:
        raise ValueError("Input values out of bounds (lidar): " + bad[0])
    cells = subcolumns(frac_out, mr_lsliq, mr_lsice, mr_cvliq, mr_cvice, dtype)
    pmol, pnorm, tautot, refl = simulate(p, t, presf, cells, (reff_lsliq, reff_lsice, reff_cvliq, reff_cvice), ice_type, dtype)
    code, _ = bin_codes(pnorm, pmol, dtype)
    out = stats(code, refl, land, pplay, dtype)
    out.update(pmol=pmol, beta_tot=pnorm, tau_tot=tautot, refl=refl, code=code)
    return out


def cfad_counts(cfad, ncol):
    """cfad_sr as whole sub-columns per cell, -1 where it is undefined"""
    f = np.asarray(cfad, np.float64)
    return np.where(f == np.float64(np.asarray(cfad).dtype.type(R_UNDEF)), -1, np.rint(f * ncol)).astype(np.int64)


def cosp_lidar_prepare(f, new, frocean, dtype):
    """geosrad_lidar's arguments as GEOS_SatsimGridComp and COSP form them from satsim_util.model_fields plus QLTOT ... RDFI and FROCEAN: presf(1)
    = 0, presf(2:) = PLE(0:LM-1) (:3672, cosp_lidar.F90:60-61); pplay = PLE(0:LM-1) (cosp_stats.F90:127); the contents clamped at 0 (:3700); no
    convective contents (:3687-3690); land = 1 where FROCEAN < 0.5 (:3548, :3584)"""
    R = np.dtype(dtype).type
    A = lambda x: np.asarray(x, dtype=R)
    ple = A(f["PLE"])
    return dict(p=A(f["PLO"]), t=A(f["T"]), presf=np.ascontiguousarray(np.concatenate([np.zeros((1, ple.shape[1]), R), ple[:-1]])),
                pplay=np.ascontiguousarray(ple[:-1]), mr_lsliq=np.maximum(A(new["QLTOT"]), R(0)), mr_lsice=np.maximum(A(new["QITOT"]), R(0)),
                mr_cvliq=None, mr_cvice=None, reff_lsliq=A(new["RDFL"]), reff_lsice=A(new["RDFI"]), reff_cvliq=None, reff_cvice=None,
                land=np.where(A(frocean) < R(0.5), R(1), R(0)).astype(R))
