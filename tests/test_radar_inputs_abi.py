"""CPU: the sixth public header, include/geosrad_radar.h, and the library's exports for it, as tests/test_lidar_abi.py does for the fifth.
No device is opened: what can be asked of an entry point without one is that it exists with the header's signature and refuses a call
before it touches anything."""
import ctypes
import os
import re
import subprocess

from tests.conftest import ROOT
from geosradiation_gridcomp_amd import _lib

HDR = os.path.join(ROOT, "include", "geosrad_radar.h")
NAMES = ["geosrad_prec_scops", "geosrad_prec_scops_dev", "geosrad_cosp_sghydro", "geosrad_cosp_sghydro_dev", "geosrad_radar_gases", "geosrad_radar_gases_dev"]
CLASSES = ["lsliq", "lsice", "lsrain", "lssnow", "cvliq", "cvice", "cvrain", "cvsnow", "lsgrpl"]          # cosp_constants' I_* order
PREC_ARGS = ["npoints", "nlev", "ncol", "ls_p_rate", "cv_p_rate", "frac_out", "prec_frac"]                # prec_scops' own argument list
SG_ARGS = ["npoints", "nlev", "ncol", "frac_out"] + ["mr_" + c for c in CLASSES] + ["prec_frac", "frac_ls", "frac_cv", "prec_ls", "prec_cv", "mr_sub", "mr_hydro_sg"]
GAS_ARGS = ["npoints", "nlev", "p", "t", "rh", "zlev", "freq", "surface_radar", "g_vol", "g_to_vol"]
U8 = lambda args: [a + "_u8" if a in ("frac_out", "prec_frac") else a for a in args]
KERNELS = ["k_prec_scops", "k_sghydro", "k_radar_gases", "k_radar_gas_path"]


def test_header_declares_the_entry_points():
    protos = _lib.radar_prototypes()
    assert sorted(protos) == sorted(NAMES) == sorted(_lib.EXPORTS_RADAR)
    order = lambda n: [p for _, p in protos[n][1]]
    assert order("geosrad_prec_scops") == ["ctx"] + PREC_ARGS and order("geosrad_prec_scops_dev") == ["ctx", "stream"] + U8(PREC_ARGS)
    assert order("geosrad_cosp_sghydro") == ["ctx"] + SG_ARGS and order("geosrad_cosp_sghydro_dev") == ["ctx", "stream"] + U8(SG_ARGS)
    assert order("geosrad_radar_gases") == ["ctx"] + GAS_ARGS and order("geosrad_radar_gases_dev") == ["ctx", "stream"] + GAS_ARGS
    assert all(ret is ctypes.c_int for ret, _ in protos.values())
    scalars = {p: t for _, ps in protos.values() for t, p in ps if t is not ctypes.c_void_p}
    assert set(scalars) == {"npoints", "nlev", "ncol", "freq", "surface_radar"}
    assert scalars.pop("freq") is ctypes.c_double and set(scalars.values()) == {ctypes.c_int}
    # every declaration cites the reference lines it replaces; the header says what it refuses, which oddities it keeps and what is left
    text = open(HDR).read()
    for cite in ("prec_scops.f:25-267", ":184-191", ":192-199", ":200-207", ":208-213", ":54-55", "cosp.F90:399-519", "GEOS_SatsimGridComp.F90:3470",
                 ":404-411", ":414-431", ":484-516", ":453-480", ":473-480", ":457-469", "GEOS_SatsimGridComp.F90:3687-3690", "quickbeam/gases.f90",
                 "math_lib.f90:96-155", "radar_simulator.f90:470-484", "cosp_radar.F90:136-144", "cosp_radar.F90:136-139", "radar_simulator.f90:478",
                 "format_input.f90:66-130", ":2858", ":3613", "GEOS_SatsimGridComp.F90:3545", "cosp_constants.F90:108-127", "cosp_types.F90:1112-1126",
                 "radar_simulator.f90:258", ":434-457", "cosp_constants.F90:39-47", "CLCALIPSO2", "CLTLIDARRADAR", "pf_to_mr", "dropped", "GEOSRAD_EINPUT",
                 "7.5 GB"):
        assert cite in text, cite
    enum = re.search(r"enum\s*\{([^}]*)\}", text).group(1)
    assert [e.strip() for e in enum.split(",")] == ["GEOSRAD_HYDRO_" + c.upper() for c in CLASSES] + ["GEOSRAD_NHYDRO"]


def test_the_new_header_list_sits_beside_the_pinned_ones():
    assert len(_lib.HEADERS) == 2 and len(_lib.HEADERS_ALL) == 4 and len(_lib.HEADERS_PUBLIC) == 5 and len(_lib.HEADERS_EVERY) == 6
    assert _lib.HEADERS_EVERY[:5] == _lib.HEADERS_PUBLIC and _lib.HEADERS_EVERY[5] == (HDR, _lib.EXPORTS_RADAR)
    others = set(_lib.all_prototypes()) | set(_lib.satsim_prototypes()) | set(_lib.misr_modis_prototypes()) | set(_lib.lidar_prototypes())
    assert not set(NAMES) & others and len(_lib.EXPORTS_LIDAR) == 3
    # the build's own check walks every header
    entry = open(os.path.join(ROOT, "__graft_entry__.py")).read()
    assert "_lib.HEADERS_EVERY" in entry
    # the Python layer finds the new entry points' parameters beside the others'
    from geosradiation_gridcomp_amd import api
    assert [p for p, _ in api._params("geosrad_cosp_sghydro")] == ["ctx"] + SG_ARGS
    assert api._params("geosrad_lidar")[0][0] == "ctx"
    assert all(hasattr(api.Context, n) for n in ("prec_scops", "prec_scops_dev", "cosp_sghydro", "cosp_sghydro_dev", "radar_gases", "radar_gases_dev"))
    assert list(api.Context.HYDRO) == CLASSES


def test_header_compiles_as_c(tmp_path):
    src = tmp_path / "use.c"
    src.write_text('#include "geosrad_radar.h"\n'
                   'int (*f1)(geosrad_ctx *, int, int, int, const void *, const void *, const void *, void *) = geosrad_prec_scops;\n'
                   'int (*f2)(geosrad_ctx *, void *, int, int, const void *, const void *, const void *, const void *, double, int, void *, void *) =\n'
                   '    geosrad_radar_gases_dev;\n'
                   'int main(void) { geosrad_ctx *c = 0; return GEOSRAD_OK + (c != 0) + (f1 == 0) + (f2 == 0) + GEOSRAD_NHYDRO - 9 + GEOSRAD_HYDRO_LSGRPL - 8; }\n')
    subprocess.check_call([os.environ.get("CC", "cc"), "-Wall", "-Werror", "-I", os.path.dirname(HDR), "-c", str(src), "-o", str(tmp_path / "use.o")])


def test_library_exports_and_refuses_without_a_context():
    L = _lib.lib()
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.SO], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (geosrad_\w+)", nm))
    assert set(NAMES) <= exported
    # the four kernels are in the gfx950 code object in both precisions
    syms = subprocess.run(["strings", "-a", _lib.SO], capture_output=True, text=True, check=True).stdout
    for k in KERNELS:
        assert re.search(rf"{len(k)}{k}IfE", syms) and re.search(rf"{len(k)}{k}IdE", syms), k
    protos = _lib.radar_prototypes()
    for name in NAMES:
        fn = getattr(L, name)
        assert fn.restype is ctypes.c_int and list(fn.argtypes) == [t for t, _ in protos[name][1]], name
        # a null context is refused with GEOSRAD_EINVAL before anything else is looked at; the argument rules need a context for their
        # message and are tests/test_gpu_radar_inputs.py's
        vals = {"npoints": 4, "nlev": 5, "ncol": 3, "freq": 94.0, "surface_radar": 0}
        assert fn(*[None if t is ctypes.c_void_p else t(vals[p]) for t, p in protos[name][1]]) == 1, name
