"""CPU: the numpy restatement of scops.f / icarus.f (tests/satsim_util.py) against tests/golden/satsim_isccp_72.npz - what the reference's
own two files, compiled unmodified in r4 and r8 (DESIGN.md 4.12 has the command lines), read and wrote on the 96 x 72 x 30 batch of
satsim_util.make_batch.  This pins the restatement, the yardstick of the GPU tests for the shapes the fixture does not hold, to the reference:
masks and seeds bitwise in both kinds, every sub-column in the reference's histogram bin, every continuous output within the fixture's
spread_* (the reference's own r4-against-r8 difference of that output)."""
import numpy as np
import pytest

from tests import satsim_util as U

KINDS = [("r4", np.float32), ("r8", np.float64)]


@pytest.fixture(scope="module")
def fx():
    return np.load(U.FIXTURE)


def test_fixture_is_the_recipe_and_a_fair_batch(fx):
    b = U.make_batch()
    for k, v in b.items():
        np.testing.assert_array_equal(fx["in_" + k], v, err_msg=k)
    assert int(fx["ncol"]) == 30 and b["cc"].shape == (72, 96)
    assert (np.diff(b["at"], axis=0) != 0).all()                      # no two equal neighbouring levels: the temperature match is continuous
    assert (b["phalf"][0] == 0).all() and (b["sunlit"] == 0).sum() == 24 and (b["cc"][:, 5::8] == 0).all()
    types = set()
    for th, thd in U.OPTION_PAIRS:
        s = f"_th{th}_d{thd}"
        b4, b8 = U.bins_of(fx["r4_boxtau" + s], fx["r4_boxptop" + s]), U.bins_of(fx["r8_boxtau" + s], fx["r8_boxptop" + s])
        assert np.array_equal(b4[0], b8[0]) and np.array_equal(b4[1], b8[1])      # the reference's two builds move no sub-column
        types |= set(zip(b4[0][b4[0] > 0].tolist(), b4[1][b4[0] > 0].tolist()))
    assert len(types) >= 38
    for th in (1, 3):      # the two search directions differ on this batch
        assert (fx[f"r8_boxptop_th{th}_d1"] != fx[f"r8_boxptop_th{th}_d2"]).sum() > 20
    for ov in (1, 2, 3):
        assert (fx[f"mask_ov{ov}"] == 2).sum() > 100 and np.array_equal(fx[f"r4_seed_ov{ov}"], fx[f"r8_seed_ov{ov}"])


@pytest.mark.parametrize("kind,dt", KINDS)
@pytest.mark.parametrize("overlap", [1, 2, 3])
def test_scops_restatement_is_bitwise(fx, kind, dt, overlap):
    mask, seed = U.scops(fx["in_seed"], fx["in_cc"], fx["in_conv"], overlap, int(fx["ncol"]), dt)
    np.testing.assert_array_equal(mask, fx[f"mask_ov{overlap}"])
    np.testing.assert_array_equal(seed, fx[f"{kind}_seed_ov{overlap}"])
    assert (seed < 0).any() and (seed > 0).any()          # both signs of Fortran's mod are in play


@pytest.mark.parametrize("kind,dt", KINDS)
@pytest.mark.parametrize("th,thd", U.OPTION_PAIRS)
def test_icarus_restatement(fx, kind, dt, th, thd):
    b = {k[3:]: fx[k] for k in fx.files if k.startswith("in_")}
    o = U.icarus(b["sunlit"], b["pfull"], b["phalf"], b["qv"], b["cc"], b["conv"], b["dtau_s"], b["dtau_c"], th, thd, 3, fx["mask_ov3"], b["skt"],
                 U.EMSFC_LW, b["at"], b["dem_s"], b["dem_c"], dt)
    s = f"_th{th}_d{thd}"
    miss = dt(U.MISSING)
    got, ref = U.bins_of(o["boxtau"], o["boxptop"]), U.bins_of(fx[f"{kind}_boxtau{s}"], fx[f"{kind}_boxptop{s}"])
    assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1])
    np.testing.assert_array_equal(o["fq_isccp"], fx[f"{kind}_fq_isccp{s}"])      # the same counts added in the same order
    for n in U.CONTINUOUS:
        r = fx[f"{kind}_{n}{s}"]
        assert o[n].dtype == r.dtype == dt
        assert np.array_equal(o[n] == miss, r == miss), n
        ok = r != miss
        d = np.abs(o[n].astype(np.float64) - r.astype(np.float64))[ok].max() if ok.any() else 0.0
        print(f"{kind} top_height {th} direction {thd} {n}: {d:.3e} of {float(fx['spread_' + n + s]):.3e}")
        assert d <= float(fx["spread_" + n + s]), (n, d)


def test_wrapper_restatement():
    """cosp_isccp_simulator.F90:58-90, cosp.F90:167-174 and SGFCLD on small inputs worked by hand"""
    for dt in (np.float32, np.float64):
        psfc = np.array([100000., 101000., 98000., 99500.], dt)
        np.testing.assert_array_equal(U.cosp_seeds(psfc, dt), [66667, 100001, 1, 50001])
        np.testing.assert_array_equal(U.cosp_seeds(psfc[:1] + dt(0.75), dt), [100000])
        t = np.array([0.5, 1 - 2e-6, 1 + 5e-6, 1 - 5e-5, U.MISSING], dt)
        o = U.cosp_finish({"fq_isccp": np.arange(49 * 2, dtype=dt).reshape(7, 7, 2), "totalcldarea": t}, dt)
        np.testing.assert_array_equal(o["totalcldarea"], np.array([0.5, 1, 1, dt(1 - 5e-5), U.MISSING], dt))
        assert o["fq_isccp"][0, 3, 1] == 6 * 14 + 3 * 2 + 1
        f = U.model_fields(U.make_batch(5, 12))
        p = U.cosp_prepare(f, dt)
        assert (p["phalf"][0] == 0).all() and np.array_equal(p["phalf"][1:], f["PLE"][:-1].astype(dt)) and p["phalf"].shape == (13, 5)
        assert np.array_equal(p["cc"], dt(0.999999) * f["FCLD"].astype(dt)) and (p["cc"] <= f["FCLD"]).all()
        m = np.zeros((3, 4, 2), np.uint8); m[1, :, 0] = [1, 2, 0, 1]; m[2, :, 1] = 2
        np.testing.assert_array_equal(U.sgfcld(m, dt), np.array([[0, 0], [1, 0], [0, 2]], dt))


def test_range_check_is_the_references():
    z = np.zeros((3, 2))
    assert not U.range_check(z, z, z, z, z, z + 1)
    for k in range(6):
        for bad in (-0.1, 1.5):
            a = [z.copy() for _ in range(6)]
            a[k][1, 1] = bad
            assert U.range_check(*a) == (bad < 0 or k not in (2, 3))      # optical depths have no upper limit
