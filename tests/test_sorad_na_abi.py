"""CPU: the C ABI of the aerosol-free Chou-Suarez shortwave fluxes - the library exports the four entry points and the header declares
them, and the GEOSRAD_SONA_* / GEOSRAD_SWCNA_* enums of include/geosrad.h (as the compiler reads them), the Python name lists and the
1-based Fortran parameters name the same slots."""
import os
import re
import subprocess

from tests.conftest import ROOT

ENTRY_POINTS = ["geosrad_sorad_na", "geosrad_sorad_na_dev", "geosrad_sw_driver_chou_na_dev", "geosrad_sw_driver_chou_na_lit_dev"]
SONA = ["FLX", "FLC", "FLXU", "FLCU", "SFCBAND"]
SWCNA = ["FSWNA", "FSCNA", "FSWUNA", "FSCUNA", "FSWBANDNA"]
FDIR = os.path.join(ROOT, "geosradiation_gridcomp_amd", "fortran")


def header_values(tmp_path, prefix):
    """{name: value} of the enumerators GEOSRAD_<prefix>_*, printed by a program that includes the header"""
    hdr = os.path.join(ROOT, "include", "geosrad.h")
    names = list(dict.fromkeys(re.findall(r"\bGEOSRAD_" + prefix + r"_(\w+)", open(hdr).read())))
    src = tmp_path / f"{prefix}_enum.c"
    src.write_text('#include <stdio.h>\n#include "geosrad.h"\nint main(void) {\n' +
                   "".join(f'    printf("{n} %d\\n", (int)GEOSRAD_{prefix}_{n});\n' for n in names) + "    return 0;\n}\n")
    exe = str(tmp_path / f"{prefix}_enum")
    subprocess.check_call([os.environ.get("CC", "cc"), "-I", os.path.dirname(hdr), str(src), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, check=True).stdout
    return {a: int(b) for a, b in (ln.split() for ln in out.splitlines())}


def test_library_exports_the_entry_points():
    from geosradiation_gridcomp_amd import _lib
    L = _lib.lib()
    hdr = open(os.path.join(ROOT, "include", "geosrad.h")).read()
    for name in ENTRY_POINTS:
        assert name in _lib.EXPORTS and hasattr(L, name), name
        assert re.search(r"\bint " + name + r"\(", hdr), name


def test_names_agree_between_header_python_and_fortran(tmp_path):
    from geosradiation_gridcomp_amd import gridcomp as G
    c90 = open(os.path.join(FDIR, "geosrad_c.F90")).read()
    g90 = open(os.path.join(FDIR, "gridcomp_shims.F90")).read()
    s90 = open(os.path.join(FDIR, "chou_shims.F90")).read()
    for prefix, names, f90 in (("SONA", SONA, c90), ("SWCNA", SWCNA, g90)):
        want = {**{n: i for i, n in enumerate(names)}, "NOUT": len(names)}
        assert header_values(tmp_path, prefix) == want, prefix
        par = {a: int(b) for a, b in re.findall(r"\b" + prefix + r"_(\w+)\s*=\s*(\d+)", f90)}
        assert par == {k: v + (k != "NOUT") for k, v in want.items()}, prefix          # 1-based mirrors
    # the Python lists: the solver's lower-case argument names with _na, the driver's internals
    assert G.SONA_OUT == ["flx_na", "flc_na", "flxu_na", "flcu_na", "flx_sfc_band_na"] and len(G.SONA_OUT) == len(SONA)
    assert G.SWCNA_OUT == SWCNA
    assert [k[:-2] for k in G.SWCNA_OUT] == ["FSW", "FSC", "FSWU", "FSCU", "FSWBAND"] and set(k[:-2] for k in G.SWCNA_OUT) <= set(G.SWC_OUT)
    for name in ENTRY_POINTS:
        assert f"bind(C, name='{name}')" in c90, name
    assert re.search(r"subroutine sw_driver_chou_na\(", g90) and re.search(r"subroutine sw_driver_chou_na_lit\(", g90)
    assert re.search(r"subroutine sorad_na \(", s90) and "public :: sorad, sorad_na" in s90
    assert "swchou_na" in open(os.path.join(FDIR, "Makefile")).read().split("DRIVERS :=")[1].splitlines()[0].split()


def test_null_context_is_refused():
    import ctypes
    from geosradiation_gridcomp_amd import _lib
    L = _lib.lib()
    ci = ctypes.c_int
    EINVAL = 1
    solver = [ci(1), ci(4), ci(8)] + [None] * 5 + [ctypes.c_double(0.0), None, None, ci(1), ci(2)] + [None] * 21 + [ci(0), None, None, None]
    assert L.geosrad_sorad_na(None, *solver) == EINVAL
    assert L.geosrad_sorad_na_dev(None, None, *solver) == EINVAL
    assert L.geosrad_sw_driver_chou_na_dev(None, None, ci(1), ci(4), None, None, ci(1), ci(2), None, None, ci(0), None, None) == EINVAL
    assert L.geosrad_sw_driver_chou_na_lit_dev(None, None, ci(1), ci(1), None, None, ci(4), None, None, ci(1), ci(2), None, None, ci(0), None,
                                               ctypes.c_uint64(0), None, None, ci(0), None) == EINVAL
