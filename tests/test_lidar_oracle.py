"""CPU: the numpy restatement of the lidar simulator (tests/lidar_util.py) against what the reference's own r4 and r8 builds wrote into
tests/golden/satsim_lidar_72.npz (tests/tools/satsim_lidar_fixture/make_fixture.py), for ice_type 0 and 1.  Discrete results - the CFAD bin
of every cell, hence the cloudy / usable decisions, the cfad_sr counts, lidarcld, cldlayer and the undefined cells - are identical in both
kinds; tau_tot, refl and parasolrefl, which hold no exp of a small argument, are the build's bit for bit where the generator found them so
(restate32exact_*), the others are within what the generator measured (restate64rel_*) in r8 and within 4 x the r4-r8 spread in r4.  The
GPU tests for shapes the fixture does not hold lean on this restatement."""
import numpy as np
import pytest

from tests import satsim_util as U
from tests import satsim_misr_modis_util as M
from tests import lidar_util as LU

NCOL = 30
KINDS = [("r4", np.float32), ("r8", np.float64)]


@pytest.fixture(scope="module")
def fx():
    f, g, h = np.load(LU.FIXTURE), np.load(U.FIXTURE), np.load(M.FIXTURE)
    d = {k: f[k] for k in f.files}
    d.update(mask=g["mask_ov3"], t=g["in_at"], reff_lsliq=h["in_rl"], reff_lsice=h["in_ri"], reff_cvliq=h["in_rlc"], reff_cvice=h["in_ric"])
    return d


def batch(fx):
    b = {k: fx["in_" + k] for k in ("p", "presf", "pplay", "mr_lsliq", "mr_lsice", "mr_cvliq", "mr_cvice", "land")}
    b.update({k: fx[k] for k in ("mask", "t", "reff_lsliq", "reff_lsice", "reff_cvliq", "reff_cvice")})
    return b


def restate(b, ice, dt):
    return LU.lidar(ice, b["p"], b["t"], b["presf"], b["pplay"], b["mask"], b["mr_lsliq"], b["mr_lsice"], b["mr_cvliq"], b["mr_cvice"], b["reff_lsliq"],
                    b["reff_lsice"], b["reff_cvliq"], b["reff_cvice"], b["land"], dt)


def test_the_fixture_is_the_recipe_and_covers_the_cases(fx):
    g = np.load(U.FIXTURE)
    b0 = {k[3:]: g[k] for k in g.files if k.startswith("in_") and k != "in_emsfc_lw"}
    hy = LU.thicken(M.make_hydro(b0), b0)
    extra = LU.make_lidar_inputs(b0)
    for k, v in (("p", extra["p"]), ("presf", extra["presf"]), ("pplay", extra["pplay"]), ("land", extra["land"]), ("mr_lsliq", hy["ql"]), ("mr_lsice", hy["qi"]),
                 ("mr_cvliq", hy["qlc"]), ("mr_cvice", hy["qic"])):
        np.testing.assert_array_equal(fx["in_" + k], v, err_msg=k)
    assert (fx["in_land"] == 1).any() and (fx["in_land"] == 0).any()
    for ice in (0, 1):
        code, cnt = fx[f"r8_code_ice{ice}"], fx[f"r8_cfad_counts_ice{ice}"]
        assert (np.where(cnt > 0, cnt, 0).sum(axis=(0, 2)) > 0).sum() >= 14
        assert (code == LU.ABOVE).any() and (code == 0).any() and (fx[f"r8_lidarcld_ice{ice}"] == LU.R_UNDEF).any()
        lay = fx[f"r8_cldlayer_ice{ice}"][:3]
        assert ((lay > 0) & (lay != LU.R_UNDEF)).any(axis=1).all()
        moved = int((fx[f"r4_code_ice{ice}"] != code).sum())
        assert moved <= 0.001 * code.size


@pytest.mark.parametrize("ice", [0, 1])
@pytest.mark.parametrize("kind,dt", KINDS)
def test_restatement_against_the_reference(fx, kind, dt, ice):
    tag = f"_ice{ice}"
    b = batch(fx)
    o = restate(b, ice, dt)
    undef = dt(LU.R_UNDEF)
    # discrete results: identical
    np.testing.assert_array_equal(o["code"], fx[f"{kind}_code{tag}"])
    np.testing.assert_array_equal(LU.cfad_counts(o["cfad_sr"], NCOL), fx[f"{kind}_cfad_counts{tag}"])
    for n in ("lidarcld", "cldlayer"):
        assert o[n].dtype == dt
        np.testing.assert_array_equal(o[n], fx[f"{kind}_{n}{tag}"], err_msg=n)
    np.testing.assert_array_equal(o["parasolrefl"] == undef, fx[f"{kind}_parasolrefl{tag}"] == undef)
    sample = fx["sample"]
    for n in ("parasolrefl", "pmol", "beta_tot", "tau_tot", "refl"):
        got = o[n][..., sample] if n in ("beta_tot", "tau_tot", "refl") else o[n]
        ref = fx[f"{kind}_{n}{tag}"]
        assert got.dtype == dt and got.shape == ref.shape, n
        ok = ref != undef
        d = np.abs(got.astype(np.float64) - ref.astype(np.float64))[ok]
        if kind == "r4":
            if bool(fx[f"restate32exact_{n}{tag}"]) and n in ("tau_tot", "refl", "parasolrefl"):
                np.testing.assert_array_equal(got, ref, err_msg=n)
            else:
                bound = 4 * float(fx[f"spread_{n}{tag}"])
                print(f"r4 ice_type {ice} {n}: max |restatement - reference| = {d.max():.3e} (bound {bound:.3e})")
                assert d.max() <= bound, (n, float(d.max()), bound)
        else:
            rel = d / np.maximum(np.abs(ref.astype(np.float64))[ok], 1e-300)
            bound = max(float(fx[f"restate64rel_{n}{tag}"]), 0.0)
            print(f"r8 ice_type {ice} {n}: max rel |restatement - reference| = {rel.max():.3e} (stored {bound:.3e})")
            assert rel.max() <= bound, (n, float(rel.max()), bound)


def test_restatement_rules():
    """what the restatement states beside the fixture: the bin codes at the edges, a level pmol disqualifies, the land rule on a fractional
    mask, NULL convective arrays as zeros, and the range check"""
    R = np.float32
    e = LU.srbval(R)
    assert len(e) == 15 and e[9] == R(30.) and e[13] == R(80.) and e[14] == R(999.999) - R(1.0)
    pmol = np.ones((1, 1), R)
    x = np.array([0.0, 0.01, np.nextafter(R(0.01), R(1)), 5.0, np.nextafter(R(5), R(9)), 80.0, 998.0, 1.0e4, -2.0, np.nan], R)[None, :, None]
    code, _ = LU.bin_codes(x, pmol, R)
    # 998.0 < xmax is in the last bin; a pnorm of 1.0e4 is not below xmax: undefined, as the reference's WHERE has it
    assert code[0, :, 0].tolist() == [0, 0, 1, 3, 4, 13, 14, LU.UNDEF_CODE, LU.NOBIN, LU.UNDEF_CODE]
    code, _ = LU.bin_codes(np.full((1, 3, 1), 2.0e-6, R), np.zeros((1, 1), R), R)
    assert (code == LU.UNDEF_CODE).all()
    st = LU.stats(np.array([[[4], [255]], [[0], [0]]], np.uint8).reshape(2, 2, 1), np.ones((5, 2, 1), R), np.array([0.25], R), np.array([[30000.], [90000.]], R), R)
    assert st["lidarcld"][0, 0] == 1.0 and st["lidarcld"][1, 0] == R(LU.R_UNDEF)
    assert (st["cfad_sr"][0, :, 0] == R(LU.R_UNDEF)).all() and st["cfad_sr"][1, 0, 0] == 1.0
    assert st["cldlayer"][:, 0].tolist() == [R(LU.R_UNDEF), R(LU.R_UNDEF), 1.0, 1.0]
    assert np.allclose(st["parasolrefl"][:, 0], 0.75 + 0.25 * 999.999)
    b0 = U.make_batch(12, 6, seed=5)
    hy = M.make_hydro(b0)
    ex = LU.make_lidar_inputs(b0)
    mask, _ = U.scops(b0["seed"], b0["cc"], b0["conv"], 3, 4, np.float32)
    args = lambda cv: (ex["p"], b0["at"], ex["presf"], ex["pplay"], mask, hy["ql"], hy["qi"], *cv[:2], hy["rl"], hy["ri"], *cv[2:], ex["land"], np.float64)
    a, z = LU.lidar(0, *args((None,) * 4)), LU.lidar(0, *args((np.zeros_like(hy["ql"]),) * 4))
    for n in LU.LIDAR_OUT:
        np.testing.assert_array_equal(a[n], z[n], err_msg=n)
    with pytest.raises(ValueError, match=": t$"):
        LU.lidar(0, ex["p"], np.zeros_like(b0["at"]), *args((None,) * 4)[2:])
