"""CPU: geosrad_obio_weights, the band bookkeeping of UPDATE_EXPORT's SOLAR TO OBIO conversion (GEOS_SolarGridComp.F90:7584-7737), against
the numpy restatement of the Fortran walk (tests/sw_obio_util.py), and the surface of the ocean-biology entry points in the header, the
library, the Python mirror and the Fortran shim."""
import ctypes
import os
import re
import numpy as np
import pytest
from tests.conftest import ROOT
from tests import sw_obio_util as U

from geosradiation_gridcomp_amd import gridcomp as G
from geosradiation_gridcomp_amd.api import GeosradError, obio_weights

NEW = ("geosrad_obio_weights", "geosrad_sw_update_obio_dev", "geosrad_sw_driver_rrtmg_obio_dev", "geosrad_sw_driver_rrtmg_obio_lit_dev")
SCHEME = {"CHOU": G.OBIO_CHOU, "RRTMG": G.OBIO_RRTMG}
NPAIRS = {"CHOU": 39, "RRTMG": 46}
DT = {4: np.float32, 8: np.float64}


@pytest.mark.parametrize("scheme", ["CHOU", "RRTMG"])
@pytest.mark.parametrize("rk", [4, 8])
def test_weights_equal_the_restatement(rk, scheme):
    w1, w2, order = U.solar_bands(scheme, DT[rk])
    pairs = U.walk(w1, w2, order, DT[rk])
    w, npairs = obio_weights(SCHEME[scheme], rk)
    nb = len(order)
    assert w.shape == (nb, 33) and npairs == len(pairs) == NPAIRS[scheme]
    ref = U.weights(pairs, nb)
    assert np.array_equal(w.view(np.uint64), ref.view(np.uint64))
    assert np.count_nonzero(w) == NPAIRS[scheme] and (w >= 0).all() and (w <= 1).all()
    # most solar bands feeding one OBIO band
    assert np.count_nonzero(w, axis=0).max() == (3 if scheme == "RRTMG" else 2)
    assert np.count_nonzero(w, axis=0).min() == 1
    # a solar band inside the OBIO range is spread completely: column sum 1 within one ulp of the real kind (the terms are rounded
    # quotients of one denominator); RRTMG band 14 (820-2600 cm-1) reaches below 2500 cm-1 = 4000 nm and keeps 100 / 1780
    ulp = float(np.finfo(DT[rk]).eps)
    sums = w.sum(axis=1)
    for ib in range(nb):
        if scheme == "RRTMG" and ib == 13:
            assert abs(sums[ib] - 100.0 / 1780.0) <= ulp * 100.0 / 1780.0, sums[ib]
        else:
            assert abs(sums[ib] - 1.0) <= ulp, (ib, sums[ib])


@pytest.mark.parametrize("rk", [4, 8])
def test_caller_bands_reproduce_rrtmg(rk):
    w, npairs = obio_weights(G.OBIO_RRTMG, rk)
    wb, nb = obio_weights(G.OBIO_BANDS, rk, bands=(G.SW_WAVENUM1, G.SW_WAVENUM2, G.SW_WVN_ORDER))
    assert nb == npairs == 46 and np.array_equal(w.view(np.uint64), wb.view(np.uint64))
    assert G.SW_WAVENUM1 == U.RRTMG_WAVENUM1 and G.SW_WAVENUM2 == U.RRTMG_WAVENUM2


def _rejected(scheme, rk, bands):
    with pytest.raises(GeosradError) as e:
        obio_weights(scheme, rk, bands=bands)
    assert e.value.rc == 1          # GEOSRAD_EINVAL
    return str(e.value)


@pytest.mark.parametrize("rk", [4, 8])
def test_rejected_inputs(rk):
    w1, w2, order = list(G.SW_WAVENUM1), list(G.SW_WAVENUM2), list(G.SW_WVN_ORDER)
    # a gap between two solar bands: band 5 starts 10 cm-1 above the end of band 4
    g1 = list(w1); g1[4] += 10.0
    assert _rejected(G.OBIO_BANDS, rk, (g1, w2, order)) == "SOLAR bands not complete and unique!"
    with pytest.raises(U.BandsError, match="SOLAR bands not complete and unique!"):
        U.walk(g1, w2, order, DT[rk])
    # a permuted order (still a permutation): the walk meets bands that do not follow one another
    perm = list(order); perm[3], perm[4] = perm[4], perm[3]
    assert _rejected(G.OBIO_BANDS, rk, (w1, w2, perm)) == "SOLAR bands not complete and unique!"
    # an order that is no permutation
    dup = list(order); dup[3] = dup[4]
    assert "permutation" in _rejected(G.OBIO_BANDS, rk, (w1, w2, dup))
    # the wrong number of bands for a built-in scheme
    assert _rejected(G.OBIO_RRTMG, rk, 13) == "wrong number of RRTMG bands!"
    assert "Chou" in _rejected(G.OBIO_CHOU, rk, 14)
    assert "nbands" in _rejected(G.OBIO_BANDS, rk, ([], [], []))
    # an empty band
    z2 = list(w2); z2[4] = w1[4]
    assert "wvn1 < wvn2" in _rejected(G.OBIO_BANDS, rk, (w1, z2, order))
    with pytest.raises(GeosradError):
        obio_weights(7, rk)
    with pytest.raises(GeosradError):
        obio_weights(G.OBIO_RRTMG, 16)


def test_symbols_exported_declared_and_lists_unchanged():
    from geosradiation_gridcomp_amd import _lib
    from geosradiation_gridcomp_amd.api import Context
    h = open(os.path.join(ROOT, "include", "geosrad.h")).read()
    L = _lib.lib()
    for name in NEW:
        assert re.search(rf"\bint\s+{name}\s*\(", h), name
        assert name in _lib.EXPORTS
        assert hasattr(L, name), name
    assert len(G.SWD_OUT) == 24 and len(G.SWC_OUT) == 13
    assert G.SWD_OBIO_OUT == ["DRBAND", "DFBAND"] and not set(G.SWD_OBIO_OUT) & set(G.SWD_OUT)
    assert re.search(r"GEOSRAD_OBIO_CHOU\s*,\s*GEOSRAD_OBIO_RRTMG\s*,\s*GEOSRAD_OBIO_BANDS", h) and re.search(r"GEOSRAD_NB_OBIO\s*=\s*33", h)
    assert (G.OBIO_CHOU, G.OBIO_RRTMG, G.OBIO_BANDS, G.NB_OBIO) == (0, 1, 2, 33)
    # EINVAL on a null context, before anything else is looked at
    d, u64 = ctypes.c_double, ctypes.c_uint64
    assert L.geosrad_sw_update_obio_dev(None, None, 4, 1, 14, None, None, None, None, None, None, None, None) == 1
    assert L.geosrad_sw_driver_rrtmg_obio_dev(None, None, 4, 72, 14, None, None, 3, 1, d(1361.0), d(1.0), 0, 1, 1, 40, 30, 1, None, None, None,
                                              None, None) == 1
    assert L.geosrad_sw_driver_rrtmg_obio_lit_dev(None, None, 4, 2, None, None, 72, 14, None, None, 3, 1, d(1361.0), d(1.0), 0, 1, 1, 40, 30, 1,
                                                  None, None, None, u64(0), None, None, 0, None, None) == 1
    for name in ("sw_update_obio_dev", "sw_driver_rrtmg_obio_dev", "sw_driver_rrtmg_obio_lit_dev"):
        assert callable(getattr(Context, name, None)), name
    F = open(os.path.join(ROOT, "geosradiation_gridcomp_amd", "fortran", "gridcomp_shims.F90")).read()
    for sub in ("sw_update_obio", "sw_driver_rrtmg_obio", "sw_driver_rrtmg_obio_lit"):
        assert re.search(rf"subroutine\s+{sub}\s*\(", F), sub
        assert re.search(rf"public\s*::.*\b{sub}\b", F), sub
    mk = open(os.path.join(ROOT, "geosradiation_gridcomp_amd", "fortran", "Makefile")).read()
    assert re.search(r"^DRIVERS\s*:=.*\bswobio\b", mk, re.M)
