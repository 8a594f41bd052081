"""CPU: the surface of geosrad_lw_driver_chou_dev (the Chou-Suarez branch of LW_Driver as one device entry point,
GEOS_IrradGridComp.F90:1781-1785, :1876-1912, :2093-2108, :3604-3663) in the C header, the Fortran shim and the Python lists, and the
synthetic GEOS fields the GPU tests of tests/test_gpu_lw_chou_driver.py are built on."""
import ctypes
import os
import re
import numpy as np
from tests.conftest import ROOT

# the batch of the GPU tests
NCOL, LM, START, CLOUDY = 300, 72, 7300, 0.6


def test_symbol_exported_and_declared():
    from geosradiation_gridcomp_amd import _lib
    h = open(os.path.join(ROOT, "include", "geosrad.h")).read()
    assert re.search(r"\bint\s+geosrad_lw_driver_chou_dev\s*\(", h)
    assert "geosrad_lw_driver_chou_dev" in _lib.EXPORTS
    L = _lib.lib()
    assert hasattr(L, "geosrad_lw_driver_chou_dev")
    assert L.geosrad_lw_driver_chou_dev(None, None, 1, 10, None, None, 1, 4, 7, 0, None) == 1     # EINVAL, null context


def test_header_fortran_and_python_orders_agree():
    from geosradiation_gridcomp_amd import gridcomp as G
    h = open(os.path.join(ROOT, "include", "geosrad.h")).read()
    enums = [re.findall(r"GEOSRAD_LWK_(\w+)", e) for e in re.findall(r"enum\s*\{([^}]*GEOSRAD_LWK_[^}]*)\}", h)]
    assert len(enums) == 3
    ins, consts, outs = enums
    assert ins[-1] == "NIN" and ins[:-1] == G.LWK_IN and len(G.LWK_IN) == 23
    assert consts[-1] == "NCONST" and [c[2:] for c in consts[:-1]] == G.LWK_CONST and len(G.LWK_CONST) == 4
    assert outs[-1] == "NOUT" and outs[:-1] == G.LWK_OUT and len(G.LWK_OUT) == 27
    assert G.LWK_OUT[:10] == G.LWK_OUT_REQUIRED
    c = G.lwk_consts()
    assert len(c) == len(G.LWK_CONST)
    assert c[G.LWK_CONST.index("KAPPA")] == (G.MAPL["RUNIV"] / G.MAPL["AIRMW"]) / G.MAPL["CP"] and c[G.LWK_CONST.index("TAUCRIT")] == 0.30
    F = open(os.path.join(ROOT, "geosradiation_gridcomp_amd", "fortran", "gridcomp_shims.F90")).read()
    for names, pre, count in ((G.LWK_IN, "LWK_", "LWK_NIN"), (G.LWK_OUT, "LWK_", "LWK_NOUT"), (G.LWK_CONST, "LWK_C_", "LWK_NCONST")):
        for i, k in enumerate(names):
            assert re.search(rf"\b{pre}{k}\s*=\s*{i + 1}\b", F), k                     # 1-based
        assert re.search(rf"\b{count}\s*=\s*{len(names)}\b", F), count
    assert re.search(r"subroutine\s+lw_driver_chou\s*\(", F)
    mk = open(os.path.join(ROOT, "geosradiation_gridcomp_amd", "fortran", "Makefile")).read()
    assert re.search(r"^DRIVERS\s*:=.*\blwchou\b", mk, re.M)


def test_geos_fields_lead_back_to_the_irrad_inputs():
    """synth.geos_chou_lw_fields against synth.chou_lw_inputs on the columns of the GPU tests, and the conditions those tests rely on"""
    from geosradiation_gridcomp_amd import synth, gridcomp as G
    inp = synth.make_columns(NCOL, LM, start=START, cloudy_frac=CLOUDY, aerosol=True)
    ch = synth.chou_lw_inputs(inp, aerosol=True)
    f = synth.geos_chou_lw_fields(inp, aerosol=True)
    assert set(G.LWK_IN) <= set(f)
    assert "TAUA" not in synth.geos_chou_lw_fields(inp, aerosol=False)
    undef = np.float32(G.MAPL["UNDEF"])
    dflt = (36.e-6, 14.e-6, 50.e-6, 50.e-6)
    planted_in_condensate = 0
    for s, (q, r) in enumerate((("QI", "RI"), ("QL", "RL"), ("QR", "RR"), ("QS", "RS"))):
        np.testing.assert_array_equal(f[q].astype(np.float32), ch["cwc"][s], err_msg=q)
        r32 = f[r].astype(np.float32)
        und = r32 == undef
        assert und.any() and not und.all()
        planted_in_condensate += int((und & (f[q] > 0)).sum())
        reff = np.where(und, np.float32(dflt[s]), r32) * np.float32(1.0e6)
        assert reff.dtype == np.float32
        want = ch["reff"][s]
        ulp = np.abs(reff.astype(np.float64) - want.astype(np.float64)) / np.spacing(want).astype(np.float64)
        assert ulp[~und].max() <= 2.0, (r, ulp[~und].max())                                  # 1e-6 * 1e6: two roundings
        np.testing.assert_array_equal(reff[und], np.float32(dflt[s]) * np.float32(1.0e6))
    assert planted_in_condensate >= 1                       # an UNDEF radius where there is condensate: the replacement matters
    fc = f["FCLD"]
    assert ((fc > 0) & (fc < 1)).any()                      # binary clouds change something
    assert (~(fc > 0).any(axis=0)).any()                    # a column without cloud: CLDTMP / CLDPRS stay UNDEF there
    assert (fc > 0).any()
    assert 1 < f["LCLDMH"] < f["LCLDLM"] <= LM
    np.testing.assert_array_equal(f["PLE"].astype(np.float32), ch["ple"])
    np.testing.assert_array_equal(f["TS"].astype(np.float32), ch["tg"][0])
    assert f["EMIS"].shape == (NCOL,) and f["RI"].shape == (LM, NCOL) and f["PLE"].shape == (LM + 1, NCOL)
