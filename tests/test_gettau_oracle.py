"""CPU: the plain-C restatement of gettau.F90 that the GPU tests compare against (tests/gettau_impl.h: per-species outputs, batch
layout) against the oracle's own statement of the same routines (oracle/chou_sw_oracle_impl.h cs_gettau: species sums;
oracle/chou_oracle_impl.h ch_getirtau), bit for bit in both precisions, on a synthetic batch and on the hand-built columns that force
every branch.  Two independent statements of each routine; neither is the code under test."""
import numpy as np
import pytest

from tests import gettau_util as U


@pytest.fixture(scope="module")
def gtref(tmp_path_factory):
    return U.build_ref(tmp_path_factory.mktemp("gettau"))


def _cases(gtref, lw=False):
    a, ict, icb = U.synth_batch(96, 33, start=777, lw=lw)
    yield "synthetic 96 x 33", a, [(0, 0), (ict, icb), (4, 7), (1, 1), (34, 34)]
    yield "hand-built", U.hand_columns(gtref), U.HAND_MODES


@pytest.mark.parametrize("rk", [4, 8])
def test_species_sums_equal_oracle_gettau(gtref, rk):
    """sum over species of taubeam / taudiff in the order the oracle adds them, asycl and ssacl: cs_gettau's, bit for bit"""
    cloudy = scaled = 0
    for what, a, modes in _cases(gtref):
        for ict, icb in modes:
            for ib in (0, 1, 2, 3):
                r = gtref.swtau(ib, a, ict, icb, rk)
                o = gtref.oracle_swtau(ib, a, ict, icb, rk)
                for mine, theirs in (("taubeam", "tauclb"), ("taudiff", "tauclf")):
                    t = r[mine]
                    np.testing.assert_array_equal(((t[0] + t[1]) + t[2]) + t[3], o[theirs], err_msg=f"{what} ib={ib} ict={ict} icb={icb} {mine}")
                np.testing.assert_array_equal(r["asycl"], o["asycl"], err_msg=f"{what} ib={ib} asycl")
                if ib:
                    np.testing.assert_array_equal(r["ssacl"], o["ssacl"], err_msg=f"{what} ib={ib} ssacl")
                cloudy += int((r["asycl"] != 1).sum())
                if ict:
                    scaled += int(((r["taudiff"].sum(axis=0) > 0) & (r["taudiff"].sum(axis=0) < gtref.swtau(ib, a, 0, 0, rk)["taudiff"].sum(axis=0))).sum())
    assert cloudy > 1000 and scaled > 500


@pytest.mark.parametrize("rk", [4, 8])
def test_getirtau_equals_oracle(gtref, rk):
    cloudy = 0
    for what, a, _ in _cases(gtref, lw=True):
        for ib in (1, 3, 4, 10):
            r, o = gtref.irtau(ib, a, rk), gtref.oracle_irtau(ib, a, rk)
            for k in ("taudiag", "tcldlyr", "enn"):
                np.testing.assert_array_equal(r[k], o[k], err_msg=f"{what} ib={ib} {k}")
            assert (r["tcldlyr"][0] == 1).all() and (r["enn"][0] == 0).all()
            cloudy += int((r["enn"] > 0).sum())
    assert cloudy > 500


@pytest.mark.parametrize("rk", [4, 8])
def test_hand_built_columns_take_every_branch(gtref, rk):
    dt = np.float32 if rk == 4 else np.float64
    a = U.hand_columns(gtref)
    free = gtref.swtau(0, a, 0, 0, rk)
    lap = gtref.swtau(0, a, 4, 7, rk)
    nir = gtref.swtau(2, a, 4, 7, rk)
    # in-cloud mode: the species' thicknesses whatever fcld is; beam = diffuse; the overlap mode never exceeds them
    assert (free["taubeam"] == free["taudiff"]).all() and (free["taudiff"][:, 0, 0] > 0).all() and a["fcld"][0, 0] == 0
    assert (lap["taudiff"] <= free["taudiff"]).all() and (lap["taubeam"] <= free["taubeam"]).all()
    # column 1: a radius <= 0 removes that species (not rain, whose radius does not enter)
    assert free["taudiff"][0, 1, 1] == 0 and free["taudiff"][1, 2, 1] == 0 and free["taudiff"][3, 3, 1] == 0 and free["taudiff"][2, 4, 1] > 0
    assert (free["taudiff"][[0, 1, 3], 9, 1] == 0).all() and free["taudiff"][2, 9, 1] > 0
    # column 2: the snow radius is capped at 112 microns ...
    s = free["taudiff"][3, :, 2] / (a["dp"][:, 2] * a["hyd"][3, :, 2]).astype(dt)
    np.testing.assert_allclose(s[[2, 3, 5, 7, 9]], s[1], rtol=4 * np.finfo(dt).eps)
    assert s[0] > s[1] and s[4] > s[1]
    # ... except in getnirtau's g4, which takes reff(k,4) itself: the asymmetry factor differs between 140 and 1000 microns there only
    a2 = {k: v.copy() for k, v in a.items()}
    a2["reff"][3, :, 2] = np.minimum(a["reff"][3, :, 2], 112.0)
    assert (gtref.swtau(0, a2, 4, 7, rk)["asycl"] == lap["asycl"]).all()
    assert (gtref.swtau(2, a2, 4, 7, rk)["asycl"][:, 2] != nir["asycl"][:, 2]).sum() >= 4
    # column 3: tauc below 0.02 is no cloud in the overlap mode (thickness 0, asycl 1), above it is
    tot = lap["taudiff"].sum(axis=0)[:, 3]
    assert (tot[[0, 6]] == 0).all() and (tot[[1, 2, 3, 4, 5, 7, 8, 9]] > 0).all()
    assert (lap["asycl"][[0, 6], 3] == 1).all() and (lap["asycl"][[1, 7], 3] < 1).all() and (free["taudiff"].sum(axis=0)[[0, 6], 3] > 0).all()
    # column 4: fcld 0.005 is no cloud, 0.011 and 1 are (asycl < 1; beside a fully covered layer of its super-layer the table scales the
    # thickness of a 1.1 % cover to zero)
    tot = lap["taudiff"].sum(axis=0)[:, 4]
    assert (tot[[0, 3, 6]] == 0).all() and (tot[[2, 5, 8]] > 0).all()
    assert (lap["asycl"][[0, 3, 6], 4] == 1).all() and (lap["asycl"][[1, 2, 4, 5, 7, 8, 9], 4] < 1).all()
    # column 8: cover without condensate; column 9: no cover in the middle super-layer
    assert (lap["taudiff"][:, :, 8] == 0).all() and (lap["asycl"][:, 8] == 1).all()
    assert (lap["taudiff"][:, 3:6, 9] == 0).all() and (free["taudiff"][:, 3:6, 9] > 0).all()
    # cosz enters the beam scaling only
    assert (lap["taudiff"][:, :, 6] == lap["taudiff"][:, :, 0]).all() and (lap["taudiff"][:, :, 7] == lap["taudiff"][:, :, 0]).all()
    assert (lap["taubeam"][:, :, 6] != lap["taubeam"][:, :, 7]).any()
    # empty super-layers: mode (1, 1) puts every layer in the low one, (11, 11) in the high one - the same maximum, the same scaling
    assert all((gtref.swtau(0, a, 1, 1, rk)[k] == gtref.swtau(0, a, 11, 11, rk)[k]).all() for k in ("taubeam", "taudiff", "asycl"))


def test_cloud_top_seed_stays_clear_of_taucrit(gtref):
    """the fields of the device-against-device check of lw_cloud_diag (tests/test_gpu_gettau.py): at most 1 % of the columns may have a
    deciding TAUIR within 2 ulp of TAUCRIT / 2.13, where the two kernels may name different cloud tops"""
    from tests.test_gpu_gettau import lw_fields, near_taucrit
    for rk in (4, 8):
        dt = np.float32 if rk == 4 else np.float64
        f = lw_fields(300, 72)
        r = gtref.lw_cloud_diag({k: v.astype(dt) for k, v in f.items() if isinstance(v, np.ndarray)}, rk)
        near = near_taucrit(r["TAUIR"], dt)
        assert near.mean() <= 0.01, near.mean()
        assert (r["CLDTMP"] == dt(1e15)).sum() >= 1 and (r["CLDTMP"] != dt(1e15)).mean() > 0.3
