"""The fp32 tolerance policy (tests/fp32_spread.py) can see what the worst-case bounds cannot (CPU only).  The r4 oracle stands in for
an fp32 device evaluation on two RRTMG_SW batches of 1024 columns; clear-sky fluxes, where the r4 and r8 oracles see the same
atmosphere.  Unchanged it passes (every ratio is 1); wrong by 1e-4, by 1e-5, or by +-3e-5 of the TOA flux on alternating levels it
fails, while the rule of tests/test_gpu_sw.py::test_sw_fluxes_match_oracle (the worst-case bound around the PIFM singularity)
accepts every one of those arrays."""
import functools
import numpy as np
import pytest
from tests import fp32_spread as S

NLAY = 72


@functools.lru_cache(maxsize=None)
def _batch(iaer):
    from geosradiation_gridcomp_amd import synth
    from oracle import clib
    inp = synth.make_columns(1024, NLAY, aerosol=True, cloudy_frac=0.6)
    o = {kind: clib.rrtmg_sw(inp, prec=kind, iaer=iaer) for kind in ("r4", "r8")}
    assert o["r4"]["rc"] == 0 and o["r8"]["rc"] == 0
    for d in o.values():
        for v in d.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
    free = ~(inp["cldf"] > 0).any(axis=0)
    return o["r4"], o["r8"], o["r8"]["swdflx"][NLAY].astype(np.float64), free


def _old_rule_accepts(x, r4, toa):
    """the fp32 branch of test_sw_fluxes_match_oracle: against the oracle of the same kind, every column <= 5e-3 of the TOA flux and at
    most 1 % of the columns above 5e-4"""
    from tests.test_gpu_sw import flux_tol
    err = np.abs(np.asarray(x, dtype=np.float64) - r4.astype(np.float64)) / flux_tol(4, toa)
    worst = err.reshape(-1, err.shape[-1]).max(axis=0)
    return worst.max() <= 10.0 and (worst > 1.0).mean() <= 0.01


def _median_ratio(x, r4, r8, toa):
    return S.spread_ratios(x, r4, r8, toa)[0.5]["ratio"]


@pytest.mark.parametrize("iaer", [0, 10])
def test_oracle_r4_unchanged_passes_with_ratio_one(iaer):
    r4, r8, toa, _ = _batch(iaer)
    for k in ("swuflxc", "swdflxc"):
        r = S.assert_within_spread(f"iaer={iaer} {k}", r4[k], r4[k], r8[k], toa)
        assert all(v["ratio"] == 1.0 and v["ref"] > v["floor"] for v in r.values()), r
    r = S.assert_within_spread(f"iaer={iaer} clear-sky divergence", S.divergence(r4["swdflxc"], r4["swuflxc"]),
                               S.divergence(r4["swdflxc"], r4["swuflxc"]), S.divergence(r8["swdflxc"], r8["swuflxc"]), toa)
    assert all(v["ratio"] == 1.0 for v in r.values()), r


@pytest.mark.parametrize("iaer", [0, 10])
def test_relative_error_1e_4_fails_the_policy_and_passes_the_old_rule(iaer):
    r4, r8, toa, _ = _batch(iaer)
    for k in ("swuflxc", "swdflxc"):
        x = r4[k].astype(np.float64) * (1.0 + 1e-4)
        print(f"iaer={iaer} {k} x (1 + 1e-4): median ratio {_median_ratio(x, r4[k], r8[k], toa):.1f}")
        with pytest.raises(AssertionError, match="above the oracle's r4 - r8 spread"):
            S.assert_within_spread(f"iaer={iaer} {k} x (1 + 1e-4)", x, r4[k], r8[k], toa)
        assert _old_rule_accepts(x, r4[k], toa)


def test_relative_error_1e_5_fails_the_policy_without_aerosols():
    r4, r8, toa, _ = _batch(0)
    for k in ("swuflxc", "swdflxc"):
        x = r4[k].astype(np.float64) * (1.0 + 1e-5)
        print(f"iaer=0 {k} x (1 + 1e-5): median ratio {_median_ratio(x, r4[k], r8[k], toa):.1f}")
        with pytest.raises(AssertionError, match="above the oracle's r4 - r8 spread"):
            S.assert_within_spread(f"iaer=0 {k} x (1 + 1e-5)", x, r4[k], r8[k], toa)
        assert _old_rule_accepts(x, r4[k], toa)


@pytest.mark.parametrize("iaer", [0, 10])
def test_level_dependent_error_fails_through_the_divergence(iaer):
    """+3e-5 of the TOA flux on the odd levels of swdflxc and -3e-5 on the even ones: a few times the oracle's spread in a flux, many
    times its spread in the difference of adjacent levels"""
    r4, r8, toa, _ = _batch(iaer)
    sign = np.where(np.arange(NLAY + 1) % 2 == 1, 1.0, -1.0)[:, None]
    x = r4["swdflxc"].astype(np.float64) + 3e-5 * sign * toa[None, :]
    with pytest.raises(AssertionError, match="above the oracle's r4 - r8 spread"):
        S.assert_within_spread(f"iaer={iaer} divergence, swdflxc +-3e-5 by level", S.divergence(x, r4["swuflxc"]),
                               S.divergence(r4["swdflxc"], r4["swuflxc"]), S.divergence(r8["swdflxc"], r8["swuflxc"]), toa)
    assert _old_rule_accepts(x, r4["swdflxc"], toa)


def test_floor_lets_a_nearly_exact_quantity_carry_one_ulp_of_noise():
    """nirr (direct beam at the surface) of the cloud-free columns: the r4 oracle is within a few 1e-8 of the TOA flux of the r8 one, less
    than fp32 resolves in a number of nirr's size.  One fp32 ulp (2^-23 relative) on top, each column pushed away from the r8 value as
    an unlucky rounding would, passes because of the floor, and only so."""
    r4, r8, toa, free = _batch(0)
    assert free.sum() >= S.MIN_COLUMNS
    a4, a8, t = r4["nirr"][free], r8["nirr"][free], toa[free]
    away = np.where(a4.astype(np.float64) >= a8, 1.0, -1.0)
    x = a4.astype(np.float64) * (1.0 + away * 2.0 ** -23)
    r = S.assert_within_spread("nirr + 1 ulp", x, a4, a8, t)
    assert any(v["floor"] > v["ref"] for v in r.values()), r
    with pytest.raises(AssertionError):
        S.assert_within_spread("nirr + 1 ulp, no floor", x, a4, a8, t, floor_units=0)


def test_no_ratio_from_fewer_than_400_columns():
    r4, r8, toa, _ = _batch(0)
    k = "swuflxc"
    with pytest.raises(ValueError, match="fewer than 400 columns"):
        S.spread_ratios(r4[k][:, :399], r4[k][:, :399], r8[k][:, :399], toa[:399])
    with pytest.raises(ValueError, match="fewer than 400 columns"):
        S.direct_ratios(r4[k][:, :399], r4[k][:, :399], toa[:399], {0.5: 1.0, 0.9: 1.0})
    S.spread_ratios(r4[k][:, :400], r4[k][:, :400], r8[k][:, :400], toa[:400])
    with pytest.raises(ValueError, match="shapes differ"):
        S.spread_ratios(r4[k], r4[k][:-1], r8[k], toa)
