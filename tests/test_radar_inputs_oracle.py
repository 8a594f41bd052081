"""CPU: the numpy restatements of tests/radar_inputs_util.py against what the reference's own Fortran wrote into
tests/golden/satsim_radar_inputs_72.npz (tests/tools/satsim_radar_fixture/make_fixture.py: llnl/prec_scops.f in r4 and r8, quickbeam's gases
and path_integral in one plain build), so that tests/test_gpu_radar_inputs.py may use them at the shapes the fixture does not hold.
The reference's sub-grid hydrometeor block is inline in cosp_iter and its sghydro is local (cosp.F90:449-519): it cannot be observed from
outside, so its restatement is held to tests/lidar_util.subcolumns - the four cloud classes, which the lidar fixture pins through the
reference's lidar_simulator - and to its own index rule; the precipitation classes' parity is unpinned."""
import numpy as np
import pytest

from tests import lidar_util as LU
from tests import radar_inputs_util as RU


@pytest.fixture(scope="module")
def b():
    return RU.load_batch()


def test_the_fixture_covers_every_branch(b):
    fx = b["fx"]
    for k in RU.COVERAGE + ["rain_dropped"]:
        assert int(fx[f"count_{k}"]) > 0, k
    assert fx["prec_frac"].dtype == np.uint8 and fx["prec_frac"].shape == b["mask"].shape == (72, 30, 96)
    assert set(np.unique(fx["prec_frac"])) == {0, 1, 2, 3} and (b["mask"] == 2).any()
    # the counts are those of the stored batch
    ls, cv = RU.rates(b["mr"], np.float32)
    pf, poss_ls, poss_cv = RU.prec_scops(ls, cv, b["mask"], np.float32, detail=True)
    cov = RU.coverage(pf, poss_ls, poss_cv, b["mask"])
    assert {k: int(fx[f"count_{k}"]) for k in RU.COVERAGE} == cov


@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_prec_scops_restatement_equals_the_reference(b, dt):
    ls, cv = RU.rates(b["mr"], dt)
    assert np.array_equal(RU.prec_scops(ls, cv, b["mask"], dt), b["fx"]["prec_frac"])


def test_cv_col_is_formed_in_the_kind():
    for ncol in (1, 19, 20, 39, 40, 64, 65, 100, 140, 65535):
        assert RU.cv_col(ncol, np.float32) == RU.cv_col(ncol, np.float64) == max(ncol // 20, 1), ncol


@pytest.mark.parametrize("kind,dt", [("r4", np.float32), ("r8", np.float64)])
@pytest.mark.parametrize("sr", [0, 1])
def test_gases_restatement_is_within_the_stored_figures(b, kind, dt, sr):
    fx = b["fx"]
    g_vol, g_to_vol = RU.radar_gases(b["p"], b["t"], b["rh"], b["zlev"], float(fx["freq"]), sr, dt)
    for n, got, ref in (("g_vol", g_vol, fx[f"{kind}_g_vol"]), ("g_to_vol", g_to_vol, fx[f"{kind}_g_to_vol_sr{sr}"])):
        rel = float((np.abs(got - ref) / np.maximum(np.abs(ref), 1e-300)).max())
        print(f"{kind} surface_radar={sr} {n}: max rel |restatement - reference| = {rel:.3e} (stored {float(fx['restate64rel_' + n]):.3e})")
        assert rel <= float(fx[f"restate64rel_{n}"]), (n, rel)
    first = g_to_vol.shape[0] - 1 if sr else 0
    assert (fx[f"{kind}_g_to_vol_sr{sr}"][first] == 0).all() and (g_to_vol[first] == 0).all()          # path_integral's empty first gate
    assert RU.gases_range_check(b["p"], b["t"], b["zlev"]) is None


@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_sghydro_restatement(b, dt):
    mask, mr = b["mask"], b["mr"]
    o = RU.sghydro(mask, mr, dt)
    assert np.array_equal(o["prec_frac"], b["fx"]["prec_frac"])
    sg = RU.expand(mask, o["mr_sub"])
    # the four cloud classes are the lidar's sub-columns on the same mask
    cells = LU.subcolumns(mask, mr[0], mr[1], mr[4], mr[5], dt)
    for c, want in zip((0, 1, 4, 5), cells):
        assert np.array_equal(sg[c], want), RU.CLASSES[c]
    ncol = mask.shape[1]
    R = np.dtype(dt).type
    assert np.array_equal(o["prec_ls"], ((o["prec_frac"] & 1) != 0).sum(axis=1).astype(R) / R(ncol))
    # the oddity: rain is placed by the cloud mask and divided by the precipitating fraction; under a clear mask it is in no sub-column
    rain = np.asarray(mr[2], dt)
    cloudy = (mask == 1).any(axis=1)
    assert (sg[2][:, :, :][np.broadcast_to((~cloudy)[:, None, :], mask.shape)] == 0).all()
    dropped = (rain > 0) & ~cloudy & (o["prec_ls"] > 0)
    assert int(dropped.sum()) == int(b["fx"]["count_rain_dropped"])
    both = (rain > 0) & cloudy & (o["prec_ls"] > 0)
    with np.errstate(all="ignore"):
        assert both.any() and np.array_equal(o["mr_sub"][2][both], (rain / o["prec_ls"])[both])
    # a None class is zero
    o2 = RU.sghydro(mask, [m if i < 4 else None for i, m in enumerate(mr)], dt)
    assert (o2["mr_sub"][4:] == 0).all() and (o2["prec_cv"] == 0).all() and np.array_equal(o2["frac_ls"], o["frac_ls"])
