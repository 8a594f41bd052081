"""CPU: the C ABI of the aerosol-free RRTMG_LW fluxes - the library exports the three entry points, and the GEOSRAD_LWNA_* enum of
include/geosrad.h (as the compiler reads it), the Python name list and the Fortran parameters name the same slots."""
import os
import re
import subprocess

from tests.conftest import ROOT

ENTRY_POINTS = ["geosrad_rrtmg_lw_na", "geosrad_rrtmg_lw_na_dev", "geosrad_lw_driver_rrtmg_na_dev"]
NAMES = ["FLXAU_INT", "FLXAD_INT", "FLAU_INT", "FLAD_INT", "FLXA_INT", "FLA_INT", "DFDTSNA", "DFDTSCNA"]


def header_values(tmp_path):
    """{name: value} of the GEOSRAD_LWNA_* enumerators, printed by a program that includes the header"""
    hdr = os.path.join(ROOT, "include", "geosrad.h")
    found = re.findall(r"\bGEOSRAD_LWNA_(\w+)", open(hdr).read())
    names = list(dict.fromkeys(found))
    src = tmp_path / "lwna_enum.c"
    src.write_text('#include <stdio.h>\n#include "geosrad.h"\nint main(void) {\n' +
                   "".join(f'    printf("{n} %d\\n", (int)GEOSRAD_LWNA_{n});\n' for n in names) + "    return 0;\n}\n")
    exe = str(tmp_path / "lwna_enum")
    subprocess.check_call([os.environ.get("CC", "cc"), "-I", os.path.dirname(hdr), str(src), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, check=True).stdout
    return {a: int(b) for a, b in (ln.split() for ln in out.splitlines())}


def test_library_exports_the_entry_points():
    from geosradiation_gridcomp_amd import _lib
    L = _lib.lib()
    for name in ENTRY_POINTS:
        assert name in _lib.EXPORTS and hasattr(L, name), name
    hdr = open(os.path.join(ROOT, "include", "geosrad.h")).read()
    for name in ENTRY_POINTS:
        assert re.search(r"\bint " + name + r"\(", hdr), name


def test_lwna_names_agree_between_header_python_and_fortran(tmp_path):
    from geosradiation_gridcomp_amd import gridcomp as G
    h = header_values(tmp_path)
    assert h == {**{n: i for i, n in enumerate(NAMES)}, "NOUT": len(NAMES)}
    assert G.LWNA_OUT == NAMES
    # every one of them is an INTERNAL Update_Flx reads when the RRTMG semantics are off
    assert set(G.LWNA_OUT) == set(G.LWU_IN_NA)
    f90 = open(os.path.join(ROOT, "geosradiation_gridcomp_amd", "fortran", "gridcomp_shims.F90")).read()
    par = {a: int(b) for a, b in re.findall(r"\bLWNA_(\w+)\s*=\s*(\d+)", f90)}
    assert par == {**{n: i + 1 for i, n in enumerate(NAMES)}, "NOUT": len(NAMES)}          # 1-based mirrors
    assert re.search(r"subroutine lw_driver_rrtmg_na\(", f90) and "bind(C, name='geosrad_lw_driver_rrtmg_na_dev')" in f90
    c90 = open(os.path.join(ROOT, "geosradiation_gridcomp_amd", "fortran", "geosrad_c.F90")).read()
    assert "bind(C, name='geosrad_rrtmg_lw_na')" in c90


def test_null_context_is_refused():
    import ctypes
    from geosradiation_gridcomp_amd import _lib
    L = _lib.lib()
    ci = ctypes.c_int
    assert L.geosrad_lw_driver_rrtmg_na_dev(None, None, ci(1), ci(4), ci(0), None, None, ci(3), ci(1), ci(1), ci(1), ci(2), None, None, ci(0),
                                            None, None, None) == 1          # GEOSRAD_EINVAL
