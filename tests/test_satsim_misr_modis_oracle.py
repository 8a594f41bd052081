"""CPU: the numpy restatement of MISR_simulator.f (tests/satsim_misr_modis_util.py) against what the reference's own r4 and r8 builds wrote
into tests/golden/satsim_misr_modis_72.npz - the batch as it is and rolled by one point - and, where the fixture has no case, against the
reference's text read by hand (nlev 2 and 3, ncol 2, an all-dark call, a sunlit last point).  The GPU tests lean on this restatement for
the shapes the fixture does not hold.

Measured when the fixture was made: the restatement equals both builds BIT FOR BIT in every output, continuous ones included (MISR has no
transcendental but the constant tauchk), so every MISR comparison here is an equality.  The MODIS restatement (modis_simulator.F90 with
the wrapper's rules) follows at the end of the file, with its own measured figures."""
import numpy as np
import pytest

from tests import satsim_util as U
from tests import satsim_misr_modis_util as M

KINDS = [("r4", np.float32), ("r8", np.float64)]
NCOL = 30


@pytest.fixture(scope="module")
def fx():
    f, g = np.load(M.FIXTURE), np.load(U.FIXTURE)
    d = {k: f[k] for k in f.files}
    d.update({k: g[k] for k in g.files if k.startswith("in_") or k == "mask_ov3"})
    return d


def batch(fx, rolled=False):
    b = {k: fx["in_" + k] for k in ("sunlit", "zfull", "at", "dtau_s", "dtau_c")}
    b["mask"] = fx["mask_ov3"]
    return {k: M.roll1(v) for k, v in b.items()} if rolled else b


def run(b, dt, **kw):
    return M.misr(b["sunlit"], b["zfull"], b["at"], b["dtau_s"], b["dtau_c"], b["mask"], M.MISSING, dt, **kw)


def test_make_hydro_is_the_fixtures(fx):
    hy = M.make_hydro({k[3:]: v for k, v in fx.items() if k.startswith("in_")})
    for k in M.HYDRO:
        assert hy[k].dtype == np.float32
        np.testing.assert_array_equal(hy[k], fx["in_" + k], err_msg=k)
    deck, cdeck = fx["in_dtau_s"] > 0, fx["in_dtau_c"] > 0
    assert (np.diff(hy["zfull"], axis=0) < 0).all() and hy["zfull"][-1].min() > 0
    for k, on in (("ql", deck), ("qi", deck), ("rl", deck), ("ri", deck), ("qlc", cdeck), ("qic", cdeck), ("rlc", cdeck), ("ric", cdeck)):
        assert (hy[k][~on] == 0).all() and (hy[k][on] >= 0).all(), k
    assert hy["rl"][deck].min() >= 5e-6 and hy["rl"][deck].max() <= 2.8e-5 and hy["ri"][deck].min() >= 8e-6 and hy["ri"][deck].max() <= 8e-5


@pytest.mark.parametrize("kind,dt", KINDS)
@pytest.mark.parametrize("rolled", [False, True])
def test_restatement_is_the_reference_bit_for_bit(fx, kind, dt, rolled):
    tag = "_rolled" if rolled else ""
    o = run(batch(fx, rolled), dt)
    for n in M.MISR_OUT:
        ref = fx[f"{kind}_{n}{tag}"]
        assert o[n].dtype == ref.dtype == dt and o[n].shape == ref.shape, n
        np.testing.assert_array_equal(o[n], ref, err_msg=n)


@pytest.mark.parametrize("kind,dt", KINDS)
def test_what_the_fixture_holds(fx, kind, dt):
    """the figures the batch was chosen for, and the reference's two oddities as the fixture shows them"""
    miss = dt(M.MISSING)
    sun = fx["in_sunlit"]
    lit, dark = sun == 1, sun != 1
    assert lit.sum() == 72 and dark[-1] and lit[0]
    fq, dist, zt, area = (fx[f"{kind}_{n}"] for n in M.MISR_OUT)
    # dark points: missing in three outputs, MISR_mean_ztop 0 - except the call's last point
    assert (fq[:, :, dark] == miss).all() and (dist[:, dark] == miss).all() and (area[dark] == miss).all()
    assert (zt[dark][:-1] == 0).all() and zt[-1] == miss
    assert not (fq[:, :, lit] == miss).any() and not (zt[lit] == miss).any()
    cnt = M.misr_counts(fq, NCOL)
    assert (area[lit] > 0).sum() == 56 and (cnt.sum(axis=(1, 2)) > 0).sum() == 13 and cnt[0].sum() == 124
    assert (dist[:, lit].sum(axis=0) == 72).all()
    # rolled: the last point (the batch's point 0) is sunlit and keeps its own value; every dark point's MISR_mean_ztop is 0
    ztr, arr = fx[f"{kind}_MISR_mean_ztop_rolled"], fx[f"{kind}_MISR_cldarea_rolled"]
    sunr = M.roll1(sun)
    assert sunr[-1] == 1 and ztr[-1] != miss and (ztr[sunr != 1] == 0).all() and (arr[sunr != 1] == miss).all()
    # the pattern matcher works on the call's first point only: point 1 differs between the two orders, every other point does not
    np.testing.assert_array_equal(ztr[1:-2], zt[2:-1])
    assert ztr[-2] == 0 and zt[-1] == miss          # the batch's dark last point, second to last after the roll
    assert abs(float(zt[1]) - 5680.75) < 0.02 and abs(float(ztr[0]) - 5979.99) < 0.02
    assert float(fx["spread_MISR_mean_ztop"]) < 1e-2 and float(fx["restate64_MISR_mean_ztop"]) == 0.0


@pytest.mark.parametrize("kind,dt", KINDS)
def test_pattern_matcher_is_sequential_in_ibox(kind, dt):
    """MISR_simulator.f:314-335 by hand on one point of five sub-columns with heights a = 2918.75, 0, b = 3237.5, 0, c = 3137.5 (single thick
    warm layers).  ibox 2 lies between a and b (closer than 500 m) and is lower than ibox 3: it becomes b.  ibox 3: its upper neighbour ibox 4
    is 0: kept.  ibox 4 lies between ibox 3 and c: it becomes c.  A second point with the same sub-columns is untouched."""
    nlev, ncol = 6, 5
    z = np.array([3300., 3200., 3100., 3000., 1000., 200.], dt)
    zfull = np.repeat(z[:, None], 2, axis=1)
    at = np.full((nlev, 2), 280., dt)
    dtau_s = np.full((nlev, 2), 8., dt)
    dtau_c = np.zeros((nlev, 2), dt)
    mask = np.zeros((nlev, ncol, 2), np.uint8)
    for ibox, lev in ((0, 3), (2, 1), (4, 2)):
        mask[lev, ibox, :] = 1
    o = M.misr(np.array([1, 1]), zfull, at, dtau_s, dtau_c, mask, M.MISSING, dt, detail=True)
    # a layer of dtau 8 between two others: 0.5 (z_k + z_k-1) - 0.5 (z_k-1 - z_k+1) / dtau
    h = lambda k: dt(0.5) * (z[k] + z[k - 1]) - dt(0.5) * (z[k - 1] - z[k + 1]) / dt(8.)
    np.testing.assert_array_equal(o["ztop"][:, 1], np.array([h(3), 0, h(1), 0, h(2)], dt))
    np.testing.assert_array_equal(o["ztop"][:, 0], np.array([h(3), h(1), h(1), h(2), h(2)], dt))
    # :424-442: the two sub-columns the matcher filled have a height and no tau: they count in the area and the mean, not in the histogram
    assert M.misr_counts(o["fq_MISR_TAU_v_CTH"], ncol)[:, :, 0].sum() == 3 and M.misr_counts(o["fq_MISR_TAU_v_CTH"], ncol)[:, :, 1].sum() == 3
    assert h(3) == 2918.75 and h(1) == 3237.5 and h(2) == 3137.5
    assert o["MISR_cldarea"][0] == sum([dt(1.) / dt(5)] * 5, dt(0)) and o["MISR_cldarea"][1] == sum([dt(1.) / dt(5)] * 3, dt(0))


@pytest.mark.parametrize("kind,dt", KINDS)
@pytest.mark.parametrize("nlev", [2, 3])
def test_small_shapes(kind, dt, nlev):
    """nlev = 2: every level is the first or the last, so the penetration height is zfull itself whatever dtau is; nlev = 3: the middle level
    alone takes the dtau >= 1 branch.  ncol = 2: the pattern matcher's loop (ibox = 2 .. ncol - 1) is empty."""
    z = np.array([[8000.], [4000.], [500.]], dt)[-nlev:]
    at = np.full((nlev, 1), 250., dt)
    dtau_s = np.full((nlev, 1), 2., dt)
    mask = np.zeros((nlev, 2, 1), np.uint8)
    mask[nlev - 2, 0, 0] = 1          # sub-column 1: one cloudy level (the middle one for nlev = 3, the top one for nlev = 2); sub-column 2 clear
    o = M.misr(np.array([1]), z, at, dtau_s, np.zeros_like(dtau_s), mask, M.MISSING, dt, detail=True)
    want = z[0, 0] if nlev == 2 else dt(0.5) * (z[1, 0] + z[0, 0]) - dt(0.5) * (z[0, 0] - z[2, 0]) / dt(2.)
    assert o["ztop"][0, 0] == want and o["ztop"][1, 0] == 0
    assert o["MISR_cldarea"][0] == dt(0.5) and o["MISR_mean_ztop"][0] == (want * dt(0.5)) / dt(0.5)
    cnt = M.misr_counts(o["fq_MISR_TAU_v_CTH"], 2)[:, :, 0]
    assert cnt.sum() == 1 and cnt[M.misr_bin(want, dt) - 1, 2] == 1          # tau = 2: class 3
    assert o["dist_model_layertops"][:, 0].sum() == nlev
    with pytest.raises(ValueError, match="ncol = 1"):
        M.misr(np.array([1]), z, at, dtau_s, np.zeros_like(dtau_s), mask[:, :1], M.MISSING, dt)


@pytest.mark.parametrize("kind,dt", KINDS)
def test_thin_cloud_fix_up(kind, dt):
    """:254-276 on single thin cold layers: tau 0.6 keeps its height, 0.3 gets -1 (the no-height bin, tau class 2), 0.1 gets 0 (not seen)"""
    nlev = 4
    z = np.array([[9000.], [6000.], [3000.], [100.]], dt)
    at = np.full((nlev, 1), 240., dt)
    dtau_s = np.array([[0.], [0.6], [0.], [0.]], dt)
    dtau_c = np.array([[0.], [0.3], [0.1], [0.]], dt)
    mask = np.zeros((nlev, 3, 1), np.uint8)
    mask[1, 0, 0] = 1; mask[1, 1, 0] = 2; mask[2, 2, 0] = 2
    o = M.misr(np.array([1]), z, at, dtau_s, dtau_c, mask, M.MISSING, dt, detail=True)
    np.testing.assert_array_equal(o["ztop"][:, 0], np.array([6000., -1., 0.], dt))
    cnt = M.misr_counts(o["fq_MISR_TAU_v_CTH"], 3)[:, :, 0]
    assert cnt.sum() == 2 and cnt[0, 1] == 1 and cnt[M.misr_bin(dt(6000.), dt) - 1, 1] == 1
    assert o["MISR_cldarea"][0] == dt(1.) / dt(3.) and o["MISR_mean_ztop"][0] == (dt(6000.) * (dt(1.) / dt(3.))) / (dt(1.) / dt(3.))


@pytest.mark.parametrize("kind,dt", KINDS)
def test_all_dark_and_sunlit_last_point(fx, kind, dt):
    b = {k: v[..., :8] for k, v in batch(fx).items()}
    miss = dt(M.MISSING)
    dark = dict(b, sunlit=np.zeros(8, np.int32))
    o = run(dark, dt)
    assert (o["fq_MISR_TAU_v_CTH"] == miss).all() and (o["dist_model_layertops"] == miss).all() and (o["MISR_cldarea"] == miss).all()
    np.testing.assert_array_equal(o["MISR_mean_ztop"], np.array([0] * 7 + [miss], dt))
    # a positive missing_value: `if (MISR_cldarea(j) .gt. 0.)` divides a dark point's mean by it - 0 / m = 0, and m / m = 1 for the last point
    o = M.misr(dark["sunlit"], b["zfull"], b["at"], b["dtau_s"], b["dtau_c"], b["mask"], 9999., dt)
    np.testing.assert_array_equal(o["MISR_mean_ztop"], np.array([0] * 7 + [1], dt))
    lastlit = dict(b, sunlit=np.array([0, 1, 0, 1, 0, 0, 0, 1], np.int32))
    o = run(lastlit, dt)
    full = run(dict(b, sunlit=np.ones(8, np.int32)), dt)
    assert o["MISR_mean_ztop"][-1] == full["MISR_mean_ztop"][-1] and (o["MISR_mean_ztop"][[0, 2, 4, 5, 6]] == 0).all()
    np.testing.assert_array_equal(o["MISR_mean_ztop"][[1, 3]], full["MISR_mean_ztop"][[1, 3]])
    # sunlit = 2 is night as well: the reference tests sunlit(j) .eq. 1
    o = run(dict(b, sunlit=np.full(8, 2, np.int32)), dt)
    assert (o["MISR_cldarea"] == miss).all()


# ---- MODIS -----------------------------------------------------------------------------------------------------------------------------
def modis_batch(fx):
    g = np.load(U.FIXTURE)
    return dict(sunlit=fx["in_sunlit"], t=fx["in_at"], p=fx["in_pfull"], ph=fx["in_phalf"], dtau_s=fx["in_dtau_s"], dtau_c=fx["in_dtau_c"], mask=fx["mask_ov3"],
                ql=fx["in_ql"], qi=fx["in_qi"], qlc=fx["in_qlc"], qic=fx["in_qic"], rl=fx["in_rl"], ri=fx["in_ri"], rlc=fx["in_rlc"], ric=fx["in_ric"],
                boxptop=g["r4_boxptop_th1_d1"])


def run_modis(b, dt):
    return M.modis(b["sunlit"], b["t"], b["p"], b["ph"], b["dtau_s"], b["dtau_c"], b["mask"], b["ql"], b["qi"], b["qlc"], b["qic"], b["rl"], b["ri"], b["rlc"],
                   b["ric"], b["boxptop"], dt)


@pytest.mark.parametrize("kind,dt", KINDS)
def test_modis_restatement_against_the_reference(fx, kind, dt):
    """Discrete results bit for bit: phases, the retrieved / not-retrieved mask, histogram counts, every R_UNDEF position.  Continuous ones:
    measured when the fixture was made - r4 bit for bit in the L2 outputs and in every mean but the three through log10 (3.5e-7 relative:
    the restatement's log10 is the float64 function rounded once); r8 within 2e-15 in the sizes and 4e-14 in the log10 means
    (restate64rel_*, which the fixture stores).  The bounds here: 0 where 0 was measured, else 4 eps of the kind for r4 and twice the stored
    figure for r8."""
    o = run_modis(modis_batch(fx), dt)
    lit = fx["in_sunlit"] > 0
    undef = dt(M.R_UNDEF)
    ref = {n: fx[f"{kind}_modis_{n}"] for n in ("phase", "ctp", "tau", "size", "mean", "hist")}
    np.testing.assert_array_equal(o["phase"][:, lit], ref["phase"])
    np.testing.assert_array_equal(o["size"][:, lit] > 0, ref["size"] > 0)
    np.testing.assert_array_equal(o["modis_hist"][::-1, 1:, :][:, :, lit], ref["hist"])
    eps = float(np.finfo(dt).eps)
    for n in ("ctp", "tau", "size"):
        g, r = o[n][:, lit], ref[n]
        np.testing.assert_array_equal(g == undef, r == undef)
        bound = 0.0 if kind == "r4" else 2 * float(fx["restate64rel_modis_" + n])
        assert (np.abs(g.astype(np.float64) - r.astype(np.float64)) <= bound * np.abs(r.astype(np.float64))).all(), n
    for i, n in enumerate(M.MODIS_MEAN):
        g, r = o["modis_mean"][i, lit].astype(np.float64), ref["mean"][i].astype(np.float64)
        bound = (4 * eps if n.startswith("logtau") else 0.0) if kind == "r4" else 2 * float(fx["restate64rel_modis_mean"][i])
        assert (np.abs(g - r) <= bound * np.abs(r)).all(), n
    # the figures the batch was chosen for
    p = ref["phase"]
    assert ((p != 0).sum(), (p == 1).sum(), (p == 2).sum(), (p == 3).sum()) == (1426, 251, 959, 216)
    assert (ref["size"] > 0).sum() == 1263 and (ref["hist"].sum(axis=2) > 0).sum() == 36
    assert float(fx["spread_modis_mean"][14]) < 0.03 and np.array_equal(fx["r4_modis_phase"], fx["r8_modis_phase"])


@pytest.mark.parametrize("kind,dt", KINDS)
def test_modis_wrapper_rules_and_range_check(fx, kind, dt):
    b = {k: (v[..., :8] if k != "sunlit" else v[:8]) for k, v in modis_batch(fx).items()}
    undef = dt(M.R_UNDEF)
    o = run_modis(b, dt)
    dark = b["sunlit"] <= 0
    assert dark.any() and (o["modis_mean"][:, dark] == undef).all() and (o["modis_hist"][:, :, dark] == undef).all() and (o["phase"][:, dark] == 0).all()
    assert all((o[n][:, dark] == undef).all() for n in ("ctp", "tau", "size")) and (o["modis_hist"][:, 0, :] == undef).all()
    assert not (o["modis_hist"][:, 1:, ~dark] == undef).any()
    alld = run_modis(dict(b, sunlit=np.zeros(8, np.int32)), dt)
    assert (alld["modis_mean"] == undef).all() and (alld["modis_hist"] == undef).all() and (alld["phase"] == 0).all()
    # sunlit = 2 is day for MODIS (sunlit > 0), where it is night for MISR (sunlit == 1)
    np.testing.assert_array_equal(run_modis(dict(b, sunlit=np.where(dark, 0, 2)), dt)["modis_mean"], o["modis_mean"])
    # the convective arrays as None are zeros
    noc = dict(b, mask=np.where(b["mask"] == 2, 1, b["mask"]).astype(np.uint8))
    z = np.zeros_like(b["t"])
    a1 = run_modis(dict(noc, dtau_c=None, qlc=None, qic=None, rlc=None, ric=None), dt)
    a2 = run_modis(dict(noc, dtau_c=z, qlc=z, qic=z, rlc=z, ric=z), dt)
    for n in a1:
        np.testing.assert_array_equal(a1[n], a2[n], err_msg=n)
    # modis_simulator.F90:202-206: a negative radius under a stratiform sub-column of a sunlit point stops, of a dark point does not
    ls = (b["mask"] == 1).any(axis=1)
    k, j = np.argwhere(ls & ~dark[None, :])[0]
    bad = dict(b, ri=b["ri"].copy()); bad["ri"][k, j] = -1e-6
    with pytest.raises(ValueError, match="reff_lsice"):
        run_modis(bad, dt)
    k, j = np.argwhere(ls & dark[None, :])[0]
    bad = dict(b, ri=b["ri"].copy()); bad["ri"][k, j] = -1e-6
    run_modis(bad, dt)
    bad = dict(b, t=b["t"].copy()); bad["t"][3, np.flatnonzero(~dark)[0]] = 0
    with pytest.raises(ValueError, match="out of bounds: t"):
        run_modis(bad, dt)


@pytest.mark.parametrize("kind,dt", KINDS)
def test_modis_one_layer_by_hand(kind, dt):
    """one point, two sub-columns, three levels: sub-column 1 a liquid layer of tau 8 and 12 microns in the middle level, sub-column 2
    clear.  tau = 8, the cloud top is where an optical depth of 1 is reached inside the layer by the trapezoidal rule of :552-554, the
    phase liquid, the size the layer's own (the observed reflectance is the prediction at 12 microns, bracketed by the trial radii 11.43
    and 13.29), cf_total 0.5"""
    R = dt
    t = np.full((3, 1), 270., R); p = np.array([[20000.], [50000.], [90000.]], R); ph = np.array([[0.], [30000.], [70000.], [100000.]], R)
    tau = np.array([[0.], [8.], [0.]], R); z = np.zeros((3, 1), R)
    mask = np.zeros((3, 2, 1), np.uint8); mask[1, 0, 0] = 1
    o = M.modis(np.array([1]), t, p, ph, tau, None, mask, np.array([[0.], [1e-4], [0.]], R), z, None, None, np.full((3, 1), 12e-6, R), z, None, None,
                np.full((2, 1), 650., R), dt)
    assert o["phase"][:, 0].tolist() == [1, 0] and o["tau"][0, 0] == R(8) and o["tau"][1, 0] == R(M.R_UNDEF)
    dx = R(1)
    want_ctp = (R(30000.) * dx + (R(70000.) - R(30000.)) * (dx * dx) / (R(2.) * R(8.))) / dx
    assert o["ctp"][0, 0] == want_ctp == R(32500.)
    assert abs(float(o["size"][0, 0]) - 12e-6) < 2e-8
    m = o["modis_mean"][:, 0]
    assert m[0] == R(0.5) and m[1] == R(0.5) and m[2] == 0 and m[3] == R(0.5) and m[4] == 0 and m[5] == 0 and m[6] == R(8) and m[14] == R(32500.)
    assert m[15] == (R(2.) / R(3.) * R(1000.)) * (o["size"][0, 0] * R(8)) / R(1)
    h = o["modis_hist"][:, :, 0]
    assert h[0, 0] == R(M.R_UNDEF) and h[6 - 2, 1 + 2] == R(0.5) and h[:, 1:].sum() == R(0.5)          # pressure bin 3 of 7 from the top, tau bin 3
