"""CPU: the third public header, include/geosrad_satsim.h, and the library's exports for it.  No device is opened: what can be asked of an
entry point without one is that it exists with the header's signature and refuses a call before it touches anything."""
import ctypes
import os
import re
import subprocess

from tests.conftest import ROOT
from geosradiation_gridcomp_amd import _lib

HDR = os.path.join(ROOT, "include", "geosrad_satsim.h")
NAMES = ["geosrad_scops", "geosrad_scops_dev", "geosrad_icarus", "geosrad_icarus_dev", "geosrad_cosp_seeds_dev", "geosrad_isccp_dev"]
ICARUS_ARGS = ["npoints", "sunlit", "nlev", "ncol", "pfull", "phalf", "qv", "cc", "conv", "dtau_s", "dtau_c", "top_height", "top_height_direction",
               "overlap", "frac_out", "skt", "emsfc_lw", "at", "dem_s", "dem_c", "fq_isccp", "totalcldarea", "meanptop", "meantaucld",
               "meanalbedocld", "meantb", "meantbclr", "boxtau", "boxptop"]


def test_header_declares_the_entry_points_in_the_references_order():
    protos = _lib.satsim_prototypes()
    assert sorted(protos) == sorted(NAMES) == sorted(_lib.EXPORTS_SATSIM)
    order = lambda n: [p for _, p in protos[n][1]]
    # icarus.f:1-33 minus debug / debugcol; scops.f:1-2 minus ncolprint
    assert order("geosrad_icarus") == ["ctx"] + ICARUS_ARGS
    assert order("geosrad_icarus_dev") == ["ctx", "stream"] + [a if a != "frac_out" else "frac_out_u8" for a in ICARUS_ARGS]
    assert order("geosrad_scops") == ["ctx", "npoints", "nlev", "ncol", "seed", "cc", "conv", "overlap", "frac_out"]
    assert order("geosrad_scops_dev") == ["ctx", "stream", "npoints", "nlev", "ncol", "seed", "cc", "conv", "overlap", "frac_out_u8"]
    assert order("geosrad_cosp_seeds_dev") == ["ctx", "stream", "npoints", "psfc", "seed"]
    assert order("geosrad_isccp_dev") == ["ctx", "stream", "npoints", "lm", "ncol", "t", "qv", "fcld", "cca", "ple", "plo", "dtau_s", "emiss", "dtau_c", "dem_c",
                                          "ts", "sunlit", "seed", "overlap", "top_height", "top_height_direction", "emsfc_lw"] + ICARUS_ARGS[20:] + ["sgfcld"]
    assert all(ret is ctypes.c_int for ret, _ in protos.values())
    scalars = {p: t for _, ps in protos.values() for t, p in ps if t is not ctypes.c_void_p}
    assert set(scalars) == {"npoints", "nlev", "ncol", "lm", "overlap", "top_height", "top_height_direction", "emsfc_lw"}
    assert scalars.pop("emsfc_lw") is ctypes.c_double and set(scalars.values()) == {ctypes.c_int}
    # every declaration cites the reference lines it replaces
    text = open(HDR).read()
    for cite in ("scops.f:1-2", "icarus.f:1-33", "cosp.F90:167-174", "cosp_isccp_simulator.F90:58-90", "GEOS_SatsimGridComp.F90:3727-3732", "congvec.f"):
        assert cite in text, cite


def test_the_other_headers_are_as_they_were():
    assert [h for h, _ in _lib.HEADERS_ALL[:2]] == [h for h, _ in _lib.HEADERS] and _lib.HEADERS_ALL[2] == (HDR, _lib.EXPORTS_SATSIM)
    assert not set(NAMES) & set(_lib.all_prototypes())


def test_header_compiles_as_c(tmp_path):
    src = tmp_path / "use.c"
    src.write_text('#include "geosrad_satsim.h"\n'
                   'int (*fn)(geosrad_ctx *, void *, int, int, int, int32_t *, const void *, const void *, int, void *) = geosrad_scops_dev;\n'
                   'int (*gn)(geosrad_ctx *, void *, int, const void *, int32_t *) = geosrad_cosp_seeds_dev;\n'
                   'int main(void) { geosrad_ctx *c = 0; return GEOSRAD_OK + (c != 0) + (fn == 0) + (gn == 0); }\n')
    subprocess.check_call([os.environ.get("CC", "cc"), "-Wall", "-Werror", "-I", os.path.dirname(HDR), "-c", str(src), "-o", str(tmp_path / "use.o")])


def test_library_exports_and_refuses_without_a_context():
    L = _lib.lib()
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.SO], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (geosrad_\w+)", nm))
    assert set(NAMES) <= exported
    # the three kernel groups are in the gfx950 code object of both precisions
    syms = subprocess.run(["strings", "-a", _lib.SO], capture_output=True, text=True, check=True).stdout
    for k in ("k_scops", "k_icarus_point", "k_icarus_box", "k_icarus_stats", "k_cosp_seeds", "k_sgfcld"):
        assert re.search(rf"{k}I[fd]E", syms) and re.search(rf"{k}IfE", syms) and re.search(rf"{k}IdE", syms), k
    protos = _lib.satsim_prototypes()
    for name in NAMES:
        fn = getattr(L, name)
        assert fn.restype is ctypes.c_int and list(fn.argtypes) == [t for t, _ in protos[name][1]], name
        # A null context is refused with GEOSRAD_EINVAL before anything else is looked at.  That is all a machine without a device can ask:
        # a context exists only on a device (geosrad_create: GEOSRAD_ENODEV), and the rules for overlap, top_height, top_height_direction,
        # nlev and ncol (satsim_check) need one for their message - tests/test_gpu_satsim.py::test_invalid_options_are_refused covers them.
        vals = {"npoints": 4, "nlev": 5, "ncol": 3, "lm": 5, "overlap": 3, "top_height": 1, "top_height_direction": 2, "emsfc_lw": 0.999}
        assert fn(*[None if t is ctypes.c_void_p else t(vals[p]) for t, p in protos[name][1]]) == 1, name
