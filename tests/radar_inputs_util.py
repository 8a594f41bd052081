"""Helpers of the radar front-end tests: the inputs of tests/golden/satsim_radar_inputs_72.npz beside the ISCCP batch (make_radar_inputs,
fixture_mask) and numpy restatements of the three deterministic pieces the radar simulator of GEOSsatsim_GridComp's COSP starts from:

    prec_scops   llnl/prec_scops.f:25-267
    sghydro      cosp.F90:399-519 with use_precipitation_fluxes = .false. (GEOS_SatsimGridComp.F90:3470)
    radar_gases  quickbeam/gases.f90 per cell and path_integral / avint (quickbeam/math_lib.f90:96-155, :160-393) per gate, as
                 radar_simulator.f90:470-484 calls them on the matrices of cosp_radar.F90:136-144

statement by statement, in the reference's operation order - numpy rounds every operation on its own, so it is un-fused.

Layouts as everywhere in the tests: C order with the point index last, the top of the atmosphere first: gridbox fields (nlev, npoints),
masks (nlev, ncol, npoints), mr_sub (9, nlev, npoints), mr_hydro_sg (9, nlev, ncol, npoints).  (COSP counts its levels from the surface:
its level k is level nlev+1-k here; prec_scops itself takes the top first, cosp.F90:404-411.)"""
import os

import numpy as np

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "satsim_radar_inputs_72.npz")
# cosp_constants.F90:39-47, the I_* order
CLASSES = ["lsliq", "lsice", "lsrain", "lssnow", "cvliq", "cvice", "cvrain", "cvsnow", "lsgrpl"]
LS_CLOUD, CV_CLOUD, LS_PREC, CV_PREC = (0, 1), (4, 5), (2, 3, 8), (6, 7)
FREQ = 94.0          # GHz: CloudSat
EDIT_LEVELS = (0, 1, 2, 70, 71)          # the levels of the ISCCP batch's mask the fixture replaces (fixture_mask)
COVERAGE = ["ls_first_%d" % k for k in (1, 3, 4, 5)] + ["cv_first_%d" % k for k in (1, 3, 4, 5)] + ["ls_below_%d" % k for k in (1, 2, 3, 4, 5)] + \
           ["cv_below_%d" % k for k in (1, 2, 3, 4, 5)] + ["both", "three_at_nlev_minus_1", "three_skipped_at_nlev", "prec_in_clear", "path_short", "path_avint"]


# ---- prec_scops ------------------------------------------------------------------------------------------------------------------
def cv_col(ncol, dtype):
    """prec_scops.f:54-55: cv_col = 0.05*ncol, a default-real product truncated by the assignment to an integer, at least 1"""
    R = np.dtype(dtype).type
    return max(int(R(0.05) * R(ncol)), 1)


def prec_scops(ls_p_rate, cv_p_rate, frac_out, dtype=np.float32, detail=False):
    """prec_scops.f:57-265.  ls_p_rate, cv_p_rate (nlev, npoints); frac_out (nlev, ncol, npoints), 0 / 1 / 2.  Returns prec_frac as bytes
    (nlev, ncol, npoints): 0 clear, 1 large-scale, 2 convective, 3 both.  The first level (:89-172) is the general level (:178-265) with
    no level above it: its possibility ONE looks at frac_out only, its THREE always has a level below (nlev >= 2).
    detail: also (poss_ls, poss_cv) (nlev, npoints): 0 no precipitation of the kind, 1 ONE (a cell of the kind's cloud in the level), 2 TWO
    (none, but precipitation of the kind in the level above), 3 THREE, 4 Four, 5 Five."""
    frac_out = np.asarray(frac_out)
    nlev, ncol, npoints = frac_out.shape
    assert nlev >= 2
    nfive = cv_col(ncol, dtype)
    out = np.zeros((nlev, ncol, npoints), np.uint8)
    poss = np.zeros((2, nlev, npoints), np.uint8)
    first_cols = (np.arange(ncol) < nfive)[:, None]
    for kind, rate, five in ((1, ls_p_rate, np.ones((ncol, 1), bool)), (2, cv_p_rate, first_cols)):
        cloud = frac_out == kind
        column = cloud.any(axis=0)                                   # frac_out_ls / frac_out_cv, :65-86
        for l in range(nlev):
            above = np.zeros((ncol, npoints), bool) if l == 0 else (out[l - 1] & kind) != 0      # prec_frac(ilev-1) .eq. kind .or. .eq. 3
            one = cloud[l] | above                                   # possibility ONE&TWO, :184-191 / :217-228
            three = cloud[l + 1] if l + 1 < nlev else np.zeros((ncol, npoints), bool)      # :192-199: only if ilev .lt. nlev
            a1, a3, a4 = one.any(axis=0), three.any(axis=0), column.any(axis=0)
            sel = np.where(a1, one, np.where(a3, three, np.where(a4, column, np.broadcast_to(five, one.shape))))
            active = np.asarray(rate[l]) > 0
            out[l] |= (np.uint8(kind) * (sel & active)).astype(np.uint8)
            poss[kind - 1, l] = np.where(active, np.where(a1, np.where(cloud[l].any(axis=0), 1, 2), np.where(a3, 3, np.where(a4, 4, 5))), 0)
    return (out, poss[0], poss[1]) if detail else out


def coverage(prec_frac, poss_ls, poss_cv, frac_out):
    """the counts make_fixture.py asserts and stores (COVERAGE)"""
    nlev = prec_frac.shape[0]
    c = {}
    for name, p in (("ls", poss_ls), ("cv", poss_cv)):
        for k in (1, 3, 4, 5):
            c[f"{name}_first_{k}"] = int((p[0] == k).sum())
        for k in (1, 2, 3, 4, 5):
            c[f"{name}_below_{k}"] = int((p[1:] == k).sum())
    c["both"] = int((prec_frac == 3).sum())
    c["three_at_nlev_minus_1"] = int((poss_ls[nlev - 2] == 3).sum() + (poss_cv[nlev - 2] == 3).sum())
    c["three_skipped_at_nlev"] = int((poss_ls[nlev - 1] >= 4).sum() + (poss_cv[nlev - 1] >= 4).sum())
    c["prec_in_clear"] = int(((prec_frac > 0) & (frac_out == 0)).sum())
    c["path_short"], c["path_avint"] = min(nlev - 1, 3), max(nlev - 4, 0)          # gates whose path has 1..3 points / more (per point)
    return c


# ---- sghydro ---------------------------------------------------------------------------------------------------------------------
def sghydro(frac_out, mr, dtype):
    """cosp.F90:404-431, :484-516.  mr: the nine gridbox contents (nlev, npoints) in CLASSES' order, None = zero.  Returns dict(prec_frac
    bytes; frac_ls, frac_cv, prec_ls, prec_cv (nlev, npoints): counts over ncol; mr_sub (9, nlev, npoints): the gridbox value over its
    fraction - frac_ls / frac_cv for the cloud classes, prec_ls / prec_cv for the precipitation classes - where that is not 0)."""
    R = np.dtype(dtype).type
    frac_out = np.asarray(frac_out)
    nlev, ncol, npoints = frac_out.shape
    z = np.zeros((nlev, npoints), R)
    m = [z if a is None else np.asarray(a, R) for a in mr]
    ls_p_rate = (m[2] + m[3]) + m[8]                                  # :404-406
    cv_p_rate = m[6] + m[7]                                           # :407-408
    pf = prec_scops(ls_p_rate, cv_p_rate, frac_out, dtype)
    cnt = lambda b: b.sum(axis=1).astype(R) / R(ncol)                 # :417-429: sums of 1., then / Ncolumns
    o = dict(prec_frac=pf, frac_ls=cnt(frac_out == 1), frac_cv=cnt(frac_out == 2), prec_ls=cnt((pf & 1) != 0), prec_cv=cnt((pf & 2) != 0))
    sub = np.zeros((9, nlev, npoints), R)
    with np.errstate(all="ignore"):
        for group, frac in ((LS_CLOUD, "frac_ls"), (CV_CLOUD, "frac_cv"), (LS_PREC, "prec_ls"), (CV_PREC, "prec_cv")):
            for c in group:
                sub[c] = np.where(o[frac] != 0, m[c] / o[frac], m[c])
    o["mr_sub"] = sub
    return o


def expand(frac_out, mr_sub):
    """sghydro%mr_hydro (9, nlev, ncol, npoints): the index rule of cosp.F90:453-480 - a stratiform cell (frac_out 1) carries the five ls
    classes, a convective one (2) the four cv classes, the precipitation classes too (by the cloud mask, not by prec_frac); else zero"""
    frac_out = np.asarray(frac_out)
    out = np.zeros((9,) + frac_out.shape, mr_sub.dtype)
    for c in range(9):
        kind = 2 if 4 <= c <= 7 else 1
        out[c] = np.where(frac_out == kind, mr_sub[c][:, None, :], 0)
    return out


# ---- gases -----------------------------------------------------------------------------------------------------------------------
# quickbeam/gases.f90:35-109: Liebe (1985) oxygen and water-vapour lines.  The reference holds them in real*8 arrays initialised from
# default-real constants, so each value is the single-precision number widened; F() says the same of every literal of the formulas.
F = lambda x: np.float64(np.float32(x))
O2 = np.array([
    (49.4523790, 0.0000001, 11.83, 0.0083, 0.0, 0.0056, 1.7), (49.9622570, 0.0000003, 10.72, 0.0085, 0.0, 0.0056, 1.7),
    (50.4742380, 0.0000009, 9.69, 0.0086, 0.0, 0.0056, 1.7), (50.9877480, 0.0000025, 8.89, 0.0087, 0.0, 0.0055, 1.7),
    (51.5033500, 0.0000061, 7.74, 0.0089, 0.0, 0.0056, 1.8), (52.0214090, 0.0000141, 6.84, 0.0092, 0.0, 0.0055, 1.8),
    (52.5423930, 0.0000310, 6.00, 0.0094, 0.0, 0.0057, 1.8), (53.0669060, 0.0000641, 5.22, 0.0097, 0.0, 0.0053, 1.9),
    (53.5957480, 0.0001247, 4.48, 0.0100, 0.0, 0.0054, 1.8), (54.1299999, 0.0002280, 3.81, 0.0102, 0.0, 0.0048, 2.0),
    (54.6711570, 0.0003918, 3.19, 0.0105, 0.0, 0.0048, 1.9), (55.2213650, 0.0006316, 2.62, 0.01079, 0.0, 0.00417, 2.1),
    (55.7838000, 0.0009535, 2.115, 0.0111, 0.0, 0.00375, 2.1), (56.2647770, 0.0005489, 0.01, 0.01646, 0.0, 0.00774, 0.9),
    (56.3378700, 0.0013440, 1.655, 0.01144, 0.0, 0.00297, 2.3), (56.9681000, 0.0017630, 1.255, 0.01181, 0.0, 0.00212, 2.5),
    (57.6124810, 0.0000213, 0.91, 0.01221, 0.0, 0.00094, 3.7), (58.3238740, 0.0000239, 0.621, 0.01266, 0.0, -0.00055, -3.1),
    (58.4465890, 0.0000146, 0.079, 0.01449, 0.0, 0.00597, 0.8), (59.1642040, 0.0000240, 0.386, 0.01319, 0.0, -0.00244, 0.1),
    (59.5909820, 0.0000211, 0.207, 0.0136, 0.0, 0.00344, 0.5), (60.3060570, 0.0000212, 0.207, 0.01382, 0.0, -0.00413, 0.7),
    (60.4347750, 0.0000246, 0.386, 0.01297, 0.0, 0.00132, -1.0), (61.1505580, 0.0000250, 0.621, 0.01248, 0.0, -0.00036, 5.8),
    (61.8001520, 0.0000230, 0.91, 0.01207, 0.0, -0.00159, 2.9), (62.4112120, 0.0000193, 1.255, 0.01171, 0.0, -0.00266, 2.3),
    (62.4862530, 0.0000152, 0.078, 0.01468, 0.0, -0.00477, 0.9), (62.9979740, 0.0000150, 1.66, 0.01139, 0.0, -0.00334, 2.2),
    (63.5685150, 0.0000109, 2.11, 0.01108, 0.0, -0.00417, 2.0), (64.1277640, 0.0007335, 2.62, 0.01078, 0.0, -0.00448, 2.0),
    (64.6789000, 0.0004635, 3.19, 0.0105, 0.0, -0.0051, 1.8), (65.2240670, 0.0002748, 3.81, 0.0102, 0.0, -0.0051, 1.9),
    (65.7647690, 0.0001530, 4.48, 0.0100, 0.0, -0.0057, 1.8), (66.3020880, 0.0000801, 5.22, 0.0097, 0.0, -0.0055, 1.8),
    (66.8368270, 0.0000395, 6.00, 0.0094, 0.0, -0.0059, 1.7), (67.3695950, 0.0000183, 6.84, 0.0092, 0.0, -0.0056, 1.8),
    (67.9008620, 0.0000080, 7.74, 0.0089, 0.0, -0.0058, 1.7), (68.4310010, 0.0000033, 8.69, 0.0087, 0.0, -0.0057, 1.7),
    (68.9603060, 0.0000013, 9.69, 0.0086, 0.0, -0.0056, 1.7), (69.4890210, 0.0000005, 10.72, 0.0085, 0.0, -0.0056, 1.7),
    (70.0173420, 0.0000002, 11.83, 0.0084, 0.0, -0.0056, 1.7), (118.7503410, 0.0000094, 0.0, 0.01592, 0.0, -0.00044, 0.9),
    (368.4983500, 0.0000679, 0.02, 0.0192, 0.6, 0.0, 1.0), (424.7631200, 0.0006380, 0.011, 0.01916, 0.6, 0.0, 1.0),
    (487.2493700, 0.0002350, 0.011, 0.0192, 0.6, 0.0, 1.0), (715.3931500, 0.0000996, 0.089, 0.0181, 0.6, 0.0, 1.0),
    (773.8387300, 0.0006710, 0.079, 0.0181, 0.6, 0.0, 1.0), (834.1453300, 0.0001800, 0.079, 0.0181, 0.6, 0.0, 1.0)], np.float32).astype(np.float64)
H2O = np.array([
    (22.2350800, 0.109, 2.143, 0.02784), (67.8139600, 0.0011, 8.73, 0.0276), (119.9959400, 0.0007, 8.347, 0.027),
    (183.3101170, 2.3, 0.653, 0.02835), (321.2256440, 0.0464, 6.156, 0.0214), (325.1529190, 1.54, 1.515, 0.027),
    (336.1870000, 0.001, 9.802, 0.0265), (380.1973720, 11.9, 1.018, 0.0276), (390.1345080, 0.0044, 7.318, 0.019),
    (437.3466670, 0.0637, 5.015, 0.0137), (439.1508120, 0.921, 3.561, 0.0164), (443.0182950, 0.194, 5.015, 0.0144),
    (448.0010750, 10.6, 1.37, 0.0238), (470.8889740, 0.33, 3.561, 0.0182), (474.6891270, 1.28, 2.342, 0.0198),
    (488.4911330, 0.253, 2.814, 0.0249), (503.5685320, 0.0374, 6.693, 0.0115), (504.4826920, 0.0125, 6.693, 0.0119),
    (556.9360020, 510.0, 0.114, 0.03), (620.7008070, 5.09, 2.15, 0.0223), (658.0065000, 0.274, 7.767, 0.03),
    (752.0332270, 250.0, 0.336, 0.0286), (841.0735950, 0.013, 8.113, 0.0141), (859.8650000, 0.133, 7.989, 0.0286),
    (899.4070000, 0.055, 7.845, 0.0286), (902.5550000, 0.038, 8.36, 0.0264), (906.2055240, 0.183, 5.039, 0.0234),
    (916.1715820, 8.56, 1.369, 0.0253), (970.3150220, 9.16, 1.842, 0.024), (987.9267640, 138.0, 0.178, 0.0286)], np.float32).astype(np.float64)


def gases(pres_mb, t, rh, f):
    """gases.f90:112-146 on float64 arrays of any one shape (f: GHz, a scalar): the two-way gaseous attenuation of a volume, dB/km"""
    pres_mb, t, rh = (np.asarray(a, np.float64)[..., None] for a in (pres_mb, t, rh))
    f = np.float64(f)
    th = F(300.) / t
    th2 = th * th
    th3, th5 = th2 * th, (th2 * th2) * th
    e = (rh * th5) / (F(41.45) * np.power(10.0, F(9.834) * th - 10.0))
    p = pres_mb / F(10.) - e
    one_th = 1.0 - th
    lines = lambda gm, v: ((1. / ((v - f) ** 2 + gm ** 2)) + (1. / ((v + f) ** 2 + gm ** 2))) * (gm * f / v)
    # term1, :117-122 with fpp_o2 :152-160 and s_o2 :172-175
    v0, a1, a2, a3, a4, a5, a6 = O2.T
    gm = a3 * (p * np.power(th, F(0.8) - a4) + F(1.1) * e * th)
    delt = a5 * p * np.power(th, a6)
    x = (v0 - f) ** 2 + gm ** 2
    fpp = lines(gm, v0) - (delt * f / v0) * (((v0 - f) / x) - ((v0 + f) / x))
    term1 = np.cumsum(fpp * (a1 * p * th3 * np.exp(a2 * one_th)), axis=-1)[..., -1:]
    # term2, :125-129
    gm0 = F(5.6E-3) * (p + F(1.1) * e) * np.power(th, F(0.8))
    a0 = F(3.07E-4)
    ap = F(1.4) * (1 - F(1.2) * np.power(f, F(1.5)) * F(1E-5)) * F(1E-10)
    term2 = (2 * a0 * (1.0 / (gm0 * (1 + (f / gm0) ** 2) * (1 + (f / F(60.)) ** 2))) + ap * p * np.power(th, F(2.5))) * f * p * th2
    # term3, :132-137 with fpp_h2o :162-170 and s_h2o :177-180
    v1, b1, b2, b3 = H2O.T
    gm = b3 * (p * np.power(th, F(0.8)) + F(4.8) * e * th)
    term3 = np.cumsum(lines(gm, v1) * (b1 * e * np.power(th, F(3.5)) * np.exp(b2 * one_th)), axis=-1)[..., -1:]
    # term4, :140-146
    term4 = (F(1.4E-6) * p + F(5.41E-5) * e * th3) * f * e * np.power(th, F(2.5))
    npp = term1 + term2 + term3 + term4
    return (F(0.182) * f * npp)[..., 0]


def avint(ftab, xtab):
    """avint (math_lib.f90:160-393) from xtab[0] to xtab[-1] on ascending abscissas, at least 4 of them, along axis 0: with a = xtab(1)
    and b = xtab(ntab) its brackets are ilo = 2 and ihi = ntab - 2 (:308-329)"""
    n = len(xtab)
    syl, s = xtab[0], np.zeros_like(xtab[0])
    for i in range(1, n - 2):          # i = ilo .. ihi, 0-based
        x1, x2, x3 = xtab[i - 1], xtab[i], xtab[i + 1]
        t1 = ftab[i - 1] / ((x1 - x2) * (x1 - x3))
        t2 = ftab[i] / ((x2 - x1) * (x2 - x3))
        t3 = ftab[i + 1] / ((x3 - x1) * (x3 - x2))
        at = t1 + t2 + t3
        bt = -(x2 + x3) * t1 - (x1 + x3) * t2 - (x1 + x2) * t3
        ct = x2 * x3 * t1 + x1 * x3 * t2 + x1 * x2 * t3
        ca, cb, cc = (at, bt, ct) if i == 1 else (0.5 * (at + ca), 0.5 * (bt + cb), 0.5 * (ct + cc))
        s = s + ca * (x2 ** 3 - syl ** 3) / 3.0 + cb * 0.5 * (x2 ** 2 - syl ** 2) + cc * (x2 - syl)
        ca, cb, cc, syl = at, bt, ct, x2
    b = xtab[-1]
    return s + ca * (b ** 3 - syl ** 3) / 3.0 + cb * 0.5 * (b ** 2 - syl ** 2) + cc * (b - syl)


def path(g_vol, hgt):
    """g_to_vol(k) = path_integral(g_vol, hgt, 1, k-1) (radar_simulator.f90:480; math_lib.f90:136-151) for every gate k along axis 0, the
    radar's first gate first: nothing for the first gate; up to 3 points f(j) |s(2) - s(1)| summed; more, avint on the sorted abscissas"""
    n = g_vol.shape[0]
    out = np.zeros_like(g_vol)
    up = hgt[0] < hgt[-1]
    for k in range(1, n):
        if k <= 3:
            dh = np.abs(hgt[1] - hgt[0])
            s = np.zeros_like(g_vol[0])
            for j in range(k):
                s = s + g_vol[j] * dh
            out[k] = s
        else:
            sl = slice(0, k) if np.all(up) else slice(k - 1, None, -1)
            out[k] = avint(g_vol[sl], hgt[sl])
    return out


def gases_range_check(p, t, zlev):
    """the device flags of geosrad_radar_gases: the array's name, or None"""
    if (np.asarray(p) <= 0).any():
        return "p"
    if (np.asarray(t) <= 0).any():
        return "t"
    if (np.diff(np.asarray(zlev), axis=0) >= 0).any():
        return "zlev"
    return None


def radar_gases(p, t, rh, zlev, freq, surface_radar, dtype):
    """g_vol, g_to_vol (nlev, npoints) in float64 from p (Pa), t (K), rh (%), zlev (m) (nlev, npoints), TOA first: the unit conversions in
    the real kind (cosp_radar.F90:136-139), widened, + 273.15 in double with the default-real literal (radar_simulator.f90:478), the gates
    counted from the radar (order_data: from the top for a spaceborne radar, from the surface for one at the surface)"""
    R = np.dtype(dtype).type
    A = lambda a: np.asarray(a, R)
    p_mb = (A(p) / R(100.0)).astype(np.float64)
    hgt = (A(zlev) / R(1000.0)).astype(np.float64)
    t_c = (A(t) - R(273.15)).astype(np.float64)
    g = gases(p_mb, t_c + F(273.15), A(rh).astype(np.float64), freq)
    if surface_radar:
        return g, path(g[::-1], hgt[::-1])[::-1]
    return g, path(g, hgt)


# ---- the fixture's batch ----------------------------------------------------------------------------------------------------------
def fixture_mask(mask_ov3, edit):
    """the ISCCP batch's overlap-3 mask with the levels EDIT_LEVELS replaced by the fixture's `mask_edit` (len(EDIT_LEVELS), ncol, npoints):
    the batch's clouds lie between levels 58 and 72, and a cloud in the first two levels and a bare level above a cloudy last one are what
    prec_scops' first-level and last-level branches need"""
    m = np.array(mask_ov3, np.uint8, copy=True)
    m[list(EDIT_LEVELS)] = edit
    return m


def make_mask_edit(mask_ov3):
    """by point j % 8: 0 stratiform and convective cloud in the first level; 1 in the second only; 4 a clear level above a last level with
    both kinds; 5 a clear last level; else the batch's own (clear at the top)"""
    nlev, ncol, npoints = mask_ov3.shape
    e = np.array(mask_ov3[list(EDIT_LEVELS)], np.uint8, copy=True)
    j = np.arange(npoints) % 8
    e[:3] = 0
    e[0][0:10, j == 0] = 1; e[0][10:13, j == 0] = 2
    e[1][3:8, j == 1] = 1; e[1][20:22, j == 1] = 2
    e[3][:, j == 4] = 0
    e[4][:, j == 4] = 0
    e[4][5:10, j == 4] = 1; e[4][15:17, j == 4] = 2
    e[4][:, j == 5] = 0
    return e


def make_radar_inputs(b, zfull, seed=20263):
    """What the radar's front end needs beside a satsim_util.make_batch() batch: rain, snow, graupel and convective rain and snow (nlev,
    npoints), float32 kg/kg, on bands of levels drawn per point - two large-scale bands and one convective band below level 40 with gaps
    between them, on seven points of eight a first-level band, on points j % 8 = 4 / 5 the last two / the last level alone after a dry one -
    rain where at > 268 K, snow where at < 278 K, graupel on every third point; rh = (2 + 90 w (l / (nlev - 1))^2 + 6 u) clip(pfull / 300 hPa, 1e-4, 1) %, w = U(0.2, 1) per point, u = U(0, 1) per cell: moist
    towards the surface, and a vapour pressure that stays below the air's where the batch is warm at 0.1 hPa; zlev = zfull (strictly decreasing)."""
    at = np.asarray(b["at"], np.float32).astype(np.float64)
    pf = np.asarray(b["pfull"], np.float32).astype(np.float64)
    nlev, npoints = at.shape
    rng = np.random.default_rng(seed)
    lev, j = np.arange(nlev)[:, None], np.arange(npoints)[None, :]
    band = lambda lo, hi: (lev >= lo) & (lev < hi)
    s1 = rng.integers(40, 60, (1, npoints)); n1 = rng.integers(1, 6, (1, npoints))
    s2 = rng.integers(55, 70, (1, npoints)); n2 = rng.integers(1, 12, (1, npoints))
    s3 = rng.integers(45, 68, (1, npoints)); n3 = rng.integers(1, 10, (1, npoints))
    ls = band(s1, s1 + n1) | band(s2, s2 + n2) | (band(0, 2) & (j % 8 != 7))
    cv = (band(s3, s3 + n3) & (j % 3 != 1)) | (band(0, 1) & (j % 4 <= 1))
    for a in (ls, cv):
        a[nlev - 3:, (j % 8 == 4)[0]] = [[False], [True], [True]]
        a[nlev - 3:, (j % 8 == 5)[0]] = [[False], [False], [True]]
    u = [rng.uniform(0, 1, at.shape) for _ in range(6)]
    amount = lambda k: 1e-5 * np.exp(4.0 * u[k])
    w = rng.uniform(0.2, 1.0, (1, npoints))
    o = dict(mr_lsrain=np.where(ls & (at > 268.0), amount(0), 0.0), mr_lssnow=np.where(ls & (at < 278.0), amount(1), 0.0),
             mr_lsgrpl=np.where(ls & (j % 3 == 0), 0.3 * amount(2), 0.0), mr_cvrain=np.where(cv & (at > 268.0), amount(3), 0.0),
             mr_cvsnow=np.where(cv & (at < 278.0), amount(4), 0.0), rh=(2.0 + 90.0 * w * (lev / (nlev - 1.0)) ** 2 + 6.0 * u[5]) * np.clip(pf / 3.0e4, 1.0e-4, 1.0), zlev=np.asarray(zfull, np.float64))
    return {k: np.ascontiguousarray(v.astype(np.float32)) for k, v in o.items()}


def load_batch():
    """the fixture's batch as the tests use it: dict(fx = the fixture's arrays; mask (nlev, ncol, npoints) bytes; mr = the nine gridbox
    contents in CLASSES' order (make_hydro()'s cloud contents, the fixture's precipitation); p, t, rh, zlev (nlev, npoints) float32)"""
    from tests import satsim_util as U
    from tests import satsim_misr_modis_util as M
    f, g, h = np.load(FIXTURE), np.load(U.FIXTURE), np.load(M.FIXTURE)
    fx = {k: f[k] for k in f.files}
    mr = [h["in_ql"], h["in_qi"], fx["in_mr_lsrain"], fx["in_mr_lssnow"], h["in_qlc"], h["in_qic"], fx["in_mr_cvrain"], fx["in_mr_cvsnow"], fx["in_mr_lsgrpl"]]
    return dict(fx=fx, mask=fixture_mask(g["mask_ov3"], fx["mask_edit"]), mr=mr, p=g["in_pfull"], t=g["in_at"], rh=fx["in_rh"], zlev=fx["in_zlev"])


def rates(mr, dtype):
    """ls_p_rate, cv_p_rate of cosp.F90:404-408 in the real kind"""
    m = [np.asarray(q, dtype) for q in mr]
    return (m[2] + m[3]) + m[8], m[6] + m[7]
