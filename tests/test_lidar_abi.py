"""CPU: the fifth public header, include/geosrad_lidar.h, and the library's exports for it, as tests/test_misr_modis_abi.py does for the
fourth.  No device is opened: what can be asked of an entry point without one is that it exists with the header's signature and refuses a
call before it touches anything."""
import ctypes
import os
import re
import subprocess

from tests.conftest import ROOT
from geosradiation_gridcomp_amd import _lib

HDR = os.path.join(ROOT, "include", "geosrad_lidar.h")
NAMES = ["geosrad_lidar", "geosrad_lidar_dev", "geosrad_cosp_lidar_dev"]
LIDAR_ARGS = ["npoints", "nlev", "ncol", "ice_type", "p", "t", "presf", "pplay", "frac_out", "mr_lsliq", "mr_lsice", "mr_cvliq", "mr_cvice", "reff_lsliq",
              "reff_lsice", "reff_cvliq", "reff_cvice", "land", "lidarcld", "cldlayer", "cfad_sr", "parasolrefl", "pmol", "beta_tot", "tau_tot", "refl"]


def test_header_declares_the_entry_points():
    protos = _lib.lidar_prototypes()
    assert sorted(protos) == sorted(NAMES) == sorted(_lib.EXPORTS_LIDAR)
    order = lambda n: [p for _, p in protos[n][1]]
    assert order("geosrad_lidar") == ["ctx"] + LIDAR_ARGS
    assert order("geosrad_lidar_dev") == ["ctx", "stream"] + [a if a != "frac_out" else "frac_out_u8" for a in LIDAR_ARGS]
    # geosrad_cosp_lidar_dev: the argument list of geosrad_cosp_dev, unchanged and in the same order, then the new inputs and the lidar's outputs
    cosp = _lib.misr_modis_prototypes()["geosrad_cosp_dev"][1]
    mine = protos["geosrad_cosp_lidar_dev"][1]
    assert mine[:len(cosp)] == cosp
    assert [p for _, p in mine[len(cosp):]] == ["frocean", "ice_type", "clcalipso", "cldlayer", "cfad_sr", "parasolrefl", "lidarpmol"]
    assert all(ret is ctypes.c_int for ret, _ in protos.values())
    scalars = {p: t for _, ps in protos.values() for t, p in ps if t is not ctypes.c_void_p}
    assert set(scalars) == {"npoints", "nlev", "ncol", "lm", "ice_type", "overlap", "top_height", "top_height_direction", "emsfc_lw"}
    assert scalars.pop("emsfc_lw") is ctypes.c_double and set(scalars.values()) == {ctypes.c_int}
    # every declaration cites the reference lines it replaces; the header says what it refuses and which oddities it keeps
    text = open(HDR).read()
    for cite in ("cosp_lidar.F90:44-82", "lidar_simulator.F90:25-415", ":419-553", "lmd_ipsl_stats.F90:34-179", "cosp_stats.F90:126-130", "cosp_stats.F90:137-140",
                 "cosp.F90:414-431", "lidar_simulator.F90:270", "cosp_simulator.F90:160-165", "GEOS_SatsimGridComp.F90:3498-3516", ":3548", ":3584", ":3672",
                 "cosp_lidar.F90:60-61", "cosp_stats.F90:127", ":3700", ":3687-3690", ":3535", "lmd_ipsl_stats.F90:249-254", "GEOS_SatsimGridComp.F90:3657",
                 "CLCALIPSO2", "CLTLIDARRADAR", "ncol = 1"):
        assert cite in text, cite
    enum = re.search(r"enum\s*\{([^}]*)\}", text).group(1)
    assert [e.strip() for e in enum.split(",")] == ["GEOSRAD_LIDAR_" + n for n in ("LOW", "MID", "HIGH", "TOTAL", "NCAT")]


def test_the_other_headers_are_as_they_were():
    assert _lib.HEADERS_PUBLIC[:4] == _lib.HEADERS_ALL and len(_lib.HEADERS_ALL) == 4 and len(_lib.HEADERS_PUBLIC) == 5
    assert _lib.HEADERS_PUBLIC[4] == (HDR, _lib.EXPORTS_LIDAR)
    assert _lib.HEADERS_ALL[2] == (_lib.HEADER_SATSIM, _lib.EXPORTS_SATSIM) and _lib.HEADERS_ALL[3] == (_lib.HEADER_MISR_MODIS, _lib.EXPORTS_MISR_MODIS)
    assert not set(NAMES) & (set(_lib.all_prototypes()) | set(_lib.satsim_prototypes()) | set(_lib.misr_modis_prototypes()))
    assert len(_lib.EXPORTS_SATSIM) == 6 and len(_lib.EXPORTS_MISR_MODIS) == 5 and len(_lib.HEADERS) == 2
    # the Python layer finds the new entry points' parameters beside the others'
    from geosradiation_gridcomp_amd import api
    assert [p for p, _ in api._params("geosrad_lidar")] == ["ctx"] + LIDAR_ARGS
    assert api._params("geosrad_cosp_dev") == api._params("geosrad_cosp_lidar_dev")[:len(api._params("geosrad_cosp_dev"))]
    assert all(hasattr(api.Context, n) for n in ("lidar", "lidar_dev", "cosp_lidar_dev"))


def test_header_compiles_as_c(tmp_path):
    src = tmp_path / "use.c"
    src.write_text('#include "geosrad_lidar.h"\n'
                   'int (*fn)(geosrad_ctx *, int, int, int, int, const void *, const void *, const void *, const void *, const void *, const void *,\n'
                   '          const void *, const void *, const void *, const void *, const void *, const void *, const void *, const void *, void *,\n'
                   '          void *, void *, void *, void *, void *, void *, void *) = geosrad_lidar;\n'
                   'int main(void) { geosrad_ctx *c = 0; return GEOSRAD_OK + (c != 0) + (fn == 0) + GEOSRAD_LIDAR_NCAT - 4; }\n')
    subprocess.check_call([os.environ.get("CC", "cc"), "-Wall", "-Werror", "-I", os.path.dirname(HDR), "-c", str(src), "-o", str(tmp_path / "use.o")])


def test_library_exports_and_refuses_without_a_context():
    L = _lib.lib()
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.SO], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (geosrad_\w+)", nm))
    assert set(NAMES) <= exported
    # the three kernels are in the gfx950 code object in both precisions
    syms = subprocess.run(["strings", "-a", _lib.SO], capture_output=True, text=True, check=True).stdout
    for k in ("k_lidar_point", "k_lidar_box", "k_lidar_stats"):
        assert re.search(rf"{k}IfE", syms) and re.search(rf"{k}IdE", syms), k
    protos = _lib.lidar_prototypes()
    for name in NAMES:
        fn = getattr(L, name)
        assert fn.restype is ctypes.c_int and list(fn.argtypes) == [t for t, _ in protos[name][1]], name
        # a null context is refused with GEOSRAD_EINVAL before anything else is looked at; the argument rules need a context for their
        # message and are tests/test_gpu_lidar.py's
        vals = {"npoints": 4, "nlev": 5, "ncol": 3, "lm": 5, "ice_type": 0, "overlap": 3, "top_height": 1, "top_height_direction": 2, "emsfc_lw": 0.999}
        assert fn(*[None if t is ctypes.c_void_p else t(vals[p]) for t, p in protos[name][1]]) == 1, name
