"""CPU: the surface of geosrad_sw_driver_rrtmg_lit_dev / geosrad_sw_driver_chou_lit_dev (the SW branch of SORADCORE on the un-packed
tile, PackIt and UnPackIt inside: GEOS_SolarGridComp.F90:3686, :3839-3894, :6520-6580) in the C header, the library, the Python mirror
and the Fortran shim."""
import ctypes
import inspect
import os
import re
from tests.conftest import ROOT

NEW = ("geosrad_sw_driver_rrtmg_lit_dev", "geosrad_sw_driver_chou_lit_dev")


def test_symbols_exported_and_declared():
    from geosradiation_gridcomp_amd import _lib
    h = open(os.path.join(ROOT, "include", "geosrad.h")).read()
    L = _lib.lib()
    for name in NEW:
        assert re.search(rf"\bint\s+{name}\s*\(", h), name
        assert name in _lib.EXPORTS
        assert hasattr(L, name), name
    # EINVAL on a null context, before anything else is looked at
    d, u64 = ctypes.c_double, ctypes.c_uint64
    assert L.geosrad_sw_driver_rrtmg_lit_dev(None, None, 4, 2, None, None, 72, 14, None, None, 3, 1, d(1361.0), d(1.0), 0, 1, 1, 40, 30, 1, None,
                                             None, None, u64(0), None) == 1
    assert L.geosrad_sw_driver_chou_lit_dev(None, None, 4, 2, None, None, 72, None, None, 30, 40, None, None, 0, None, u64(0), None) == 1


def test_python_mirror_has_both_wrappers():
    from geosradiation_gridcomp_amd.api import Context
    for name, packed in (("sw_driver_rrtmg_lit_dev", "sw_driver_rrtmg_dev"), ("sw_driver_chou_lit_dev", "sw_driver_chou_dev")):
        assert callable(getattr(Context, name, None)), name
        got = list(inspect.signature(getattr(Context, name)).parameters)
        assert got[:6] == ["self", "stream", "ncol", "nlit", "lit_index", "lit_pos"] and got[-2:] == ["dark", "keep"]
        # between them: the packed wrapper's arguments in its order
        assert got[6:-2] == list(inspect.signature(getattr(Context, packed)).parameters)[3:], name


def test_header_fortran_and_python_orders_agree():
    from geosradiation_gridcomp_amd import gridcomp as G
    h = open(os.path.join(ROOT, "include", "geosrad.h")).read()
    F = open(os.path.join(ROOT, "geosradiation_gridcomp_amd", "fortran", "gridcomp_shims.F90")).read()
    for tag, lists in (("SWD", (G.SWD_IN, G.SWD_CONST, G.SWD_OUT)), ("SWC", (G.SWC_IN, G.SWC_CONST, G.SWC_OUT))):
        enums = [re.findall(rf"GEOSRAD_{tag}_(\w+)", re.sub(r"/\*.*?\*/", "", e, flags=re.S))
                 for e in re.findall(rf"enum\s*\{{([^}}]*GEOSRAD_{tag}_[^}}]*)\}}", h)]
        assert len(enums) == 3, tag
        ins, consts, outs = enums
        assert ins[-1] == "NIN" and ins[:-1] == lists[0], tag
        assert consts[-1] == "NCONST" and [c[2:] for c in consts[:-1]] == lists[1], tag
        assert outs[-1] == "NOUT" and outs[:-1] == lists[2], tag
        assert len(lists[2]) <= 64                                      # one keep bit per output in a uint64_t
        for names, pre, count in ((lists[0], f"{tag}_", f"{tag}_NIN"), (lists[2], f"{tag}_", f"{tag}_NOUT"), (lists[1], f"{tag}_C_", f"{tag}_NCONST")):
            for i, k in enumerate(names):
                assert re.search(rf"\b{pre}{k}\s*=\s*{i + 1}\b", F), k          # 1-based
            assert re.search(rf"\b{count}\s*=\s*{len(names)}\b", F), count
    assert len(G.SWD_OUT) == 24 and len(G.SWC_OUT) == 13
    for sub in ("sw_driver_rrtmg_lit", "sw_driver_chou_lit"):
        assert re.search(rf"subroutine\s+{sub}\s*\(", F), sub
        assert re.search(rf"public\s*::.*\b{sub}\b", F), sub
    mk = open(os.path.join(ROOT, "geosradiation_gridcomp_amd", "fortran", "Makefile")).read()
    assert re.search(r"^DRIVERS\s*:=.*\bswlit\b", mk, re.M)
    assert os.path.exists(os.path.join(ROOT, "geosradiation_gridcomp_amd", "fortran", "swlit_driver.F90"))
