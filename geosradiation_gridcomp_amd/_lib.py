"""Loader for the C-ABI shared library (include/geosrad.h) and its build recipe.

The product has no CPU path: if libgeosrad.so cannot be loaded, or no HIP device is visible, everything
here raises.  (oracle/ is test infrastructure and is never imported from this package.)
"""
import ctypes
import functools
import os
import re
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
SO = os.environ.get("GEOSRAD_LIB") or os.path.join(CSRC, "libgeosrad.so")   # override only for A/B kernel experiments
DATA = os.path.join(HERE, "data")
HEADER = os.path.join(os.path.dirname(HERE), "include", "geosrad.h")    # the one statement of every entry point's argument order and types
HEADER_GETTAU = os.path.join(os.path.dirname(HERE), "include", "geosrad_gettau.h")      # gettau.F90 as batched entry points: a second public header

EXPORTS = [
    "geosrad_create", "geosrad_create_multi", "geosrad_pick_device", "geosrad_destroy", "geosrad_last_error", "geosrad_real_kind", "geosrad_set_chunk",
    "geosrad_workspace_bytes", "geosrad_set_tables_lw", "geosrad_load_tables_lw", "geosrad_set_inhomogeneity",
    "geosrad_load_inhomogeneity", "geosrad_set_corr_lengths", "geosrad_rrtmg_lw", "geosrad_rrtmg_lw_dev",
    "geosrad_check", "geosrad_profile", "geosrad_profile_read", "geosrad_kernel_name", "geosrad_kernel_label", "geosrad_rrtmg_lw_taumol", "geosrad_mcica", "geosrad_clearcounts",
    "geosrad_set_tables_sw", "geosrad_load_tables_sw", "geosrad_rrtmg_sw", "geosrad_rrtmg_sw_dev", "geosrad_rrtmg_sw_taumol", "geosrad_mcica_dev",
    "geosrad_set_tables_chou_lw", "geosrad_load_tables_chou_lw", "geosrad_irrad", "geosrad_irrad_dev",
    "geosrad_lw_driver_rrtmg_dev", "geosrad_sw_driver_rrtmg_dev", "geosrad_lw_update_flx_dev", "geosrad_sw_update_export_dev",
    "geosrad_rad_tendencies_dev", "geosrad_lw_chou_post_dev", "geosrad_sw_driver_chou_dev", "geosrad_rrtmg_lw_rats_dev", "geosrad_lw_driver_rrtmg_rats_dev", "geosrad_lw_update_rats_dev", "geosrad_lw_update_bands_dev", "geosrad_sw_update_surface_dev",
    "geosrad_sw_update_clouds_dev", "geosrad_sw_update_cldhb_dev", "geosrad_lw_driver_chou_dev",
    "geosrad_set_tables_chou_sw", "geosrad_load_tables_chou_sw", "geosrad_sorad", "geosrad_sorad_dev",
    "geosrad_read_table", "geosrad_rrtmg_sw_cldprmc", "geosrad_set_overcast", "geosrad_get_overcast", "geosrad_lit_index_dev", "geosrad_lit_pack_dev", "geosrad_lit_unpack_dev", "geosrad_dbg_fast64",
    "geosrad_rrtmg_sw_radval", "geosrad_rrtmg_sw_radval_dev",
    "geosrad_sw_driver_rrtmg_lit_dev", "geosrad_sw_driver_chou_lit_dev",
    "geosrad_obio_weights", "geosrad_sw_update_obio_dev", "geosrad_sw_driver_rrtmg_obio_dev", "geosrad_sw_driver_rrtmg_obio_lit_dev",
    "geosrad_rrtmg_lw_na", "geosrad_rrtmg_lw_na_dev", "geosrad_lw_driver_rrtmg_na_dev",
    "geosrad_sorad_na", "geosrad_sorad_na_dev", "geosrad_sw_driver_chou_na_dev", "geosrad_sw_driver_chou_na_lit_dev",
]

# the entry points of include/geosrad_gettau.h
EXPORTS_GETTAU = [
    "geosrad_getvistau", "geosrad_getvistau_dev", "geosrad_getnirtau", "geosrad_getnirtau_dev", "geosrad_getirtau", "geosrad_getirtau_dev",
    "geosrad_lw_cloud_diag_dev",
]
HEADERS = [(HEADER, EXPORTS), (HEADER_GETTAU, EXPORTS_GETTAU)]      # the radiation headers with the names they must declare

# the satellite simulator's ISCCP path: the third public header, include/geosrad_satsim.h, with its entry points.  It is bound beside
# HEADERS / all_prototypes (satsim_prototypes, HEADERS_ALL; api._params looks in both) and not inside them, because tests/test_gettau_binding.py
# pins HEADERS to the two radiation headers and all_prototypes to their names, and existing tests stay as they are
HEADER_SATSIM = os.path.join(os.path.dirname(HERE), "include", "geosrad_satsim.h")
EXPORTS_SATSIM = [
    "geosrad_scops", "geosrad_scops_dev", "geosrad_icarus", "geosrad_icarus_dev", "geosrad_cosp_seeds_dev", "geosrad_isccp_dev",
]
# the MISR and MODIS simulators and the whole COSP path: the fourth public header, include/geosrad_misr_modis.h, bound beside the others for the
# same reason - tests/test_satsim_abi.py pins geosrad_satsim.h to its six names
HEADER_MISR_MODIS = os.path.join(os.path.dirname(HERE), "include", "geosrad_misr_modis.h")
EXPORTS_MISR_MODIS = ["geosrad_misr", "geosrad_misr_dev", "geosrad_modis", "geosrad_modis_dev", "geosrad_cosp_dev"]
HEADERS_ALL = HEADERS + [(HEADER_SATSIM, EXPORTS_SATSIM), (HEADER_MISR_MODIS, EXPORTS_MISR_MODIS)]      # the four headers before the lidar's
# the lidar simulator and the COSP path with it: the fifth public header, include/geosrad_lidar.h, bound beside the others for the same
# reason - tests/test_misr_modis_abi.py pins geosrad_misr_modis.h to its five names and HEADERS_ALL to four headers, so the list of every
# public header has a name of its own
HEADER_LIDAR = os.path.join(os.path.dirname(HERE), "include", "geosrad_lidar.h")
EXPORTS_LIDAR = ["geosrad_lidar", "geosrad_lidar_dev", "geosrad_cosp_lidar_dev"]
HEADERS_PUBLIC = HEADERS_ALL + [(HEADER_LIDAR, EXPORTS_LIDAR)]      # the five headers before the radar's
# the radar simulator's front end: the sixth public header, include/geosrad_radar.h, bound beside the others for the same reason -
# tests/test_lidar_abi.py pins HEADERS_PUBLIC to five headers, so the list of every public header has a new name again
HEADER_RADAR = os.path.join(os.path.dirname(HERE), "include", "geosrad_radar.h")
EXPORTS_RADAR = ["geosrad_prec_scops", "geosrad_prec_scops_dev", "geosrad_cosp_sghydro", "geosrad_cosp_sghydro_dev", "geosrad_radar_gases",
                 "geosrad_radar_gases_dev"]
HEADERS_EVERY = HEADERS_PUBLIC + [(HEADER_RADAR, EXPORTS_RADAR)]      # every public header

_lib = None


def build(force=False):
    """hipcc --offload-arch=gfx950 (cross-compiles without a GPU).  Objects (compiled in parallel, each rebuilt only when one of
    the files it includes is newer): geosrad.hip three times - fp32 kernels, fp64 kernels, the extern "C" layer of the six public headers; it
    includes gettau_kernels.hpp, satsim_kernels.hpp, misr_modis_kernels.hpp, lidar_kernels.hpp and radar_kernels.hpp like every solver's kernels - and lw_cols.hip (the
    on-chip RRTMG_LW band sweeps) and sw_reform.hip (the default RRTMG_SW band sweeps) twice each - fp32, fp64."""
    hpp = {f: os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".hpp")}
    cols_only = {"lw_cols_kernels.hpp", "sw_reform_kernels.hpp", "lw_split_kernels.hpp"}      # headers geosrad.hip does not include
    # geosrad.hip includes the six public headers and gettau_kernels.hpp, satsim_kernels.hpp, misr_modis_kernels.hpp, lidar_kernels.hpp, radar_kernels.hpp (with every other .hpp but cols_only): an edit of either rebuilds it
    deps_main = [os.path.join(CSRC, "geosrad.hip"), HEADER, HEADER_GETTAU, HEADER_SATSIM, HEADER_MISR_MODIS, HEADER_LIDAR, HEADER_RADAR] + [p for f, p in hpp.items() if f not in cols_only]
    lw_layers = ("lw_layer_down.hpp", "lw_layer_up.hpp")      # the layer bodies lw_kernels.hpp includes (twice each)
    deps_cols = [os.path.join(CSRC, "lw_cols.hip")] + [hpp[f] for f in ("lw_cols_kernels.hpp", "lw_cols.hpp", "lw_kernels.hpp", "lw_device.hpp") + lw_layers]
    deps_split = [os.path.join(CSRC, "lw_split.hip")] + [hpp[f] for f in ("lw_split_kernels.hpp", "lw_split.hpp", "lw_kernels.hpp", "lw_device.hpp") + lw_layers]
    deps_swq = [os.path.join(CSRC, "sw_reform.hip")] + [hpp[f] for f in ("sw_reform_kernels.hpp", "sw_reform.hpp", "sw_kernels.hpp", "lw_kernels.hpp", "lw_device.hpp") + lw_layers]
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    objdir = os.path.join(os.path.dirname(HERE), "build", "obj")
    os.makedirs(objdir, exist_ok=True)
    # -fno-slp-vectorize: the SLP vectorizer pairs the fp32 arithmetic of neighbouring g-points into v_pk_* instructions, which issue at half
    # the rate of the plain ones on gfx950 (profiles/tools/ubench/valu_rate.hip: v_pk_fma_f32 4.9 against v_fma_f32 2.4 cycles) and need their
    # operands moved into register pairs: the SW sweeps lose a third of their instructions and 30 VGPRs without it
    flags = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-fno-slp-vectorize"]
    units = [("geosrad.hip", part, deps_main) for part in (4, 8, 0)] + [("lw_cols.hip", part, deps_cols) for part in (4, 8)] \
        + [("sw_reform.hip", part, deps_swq) for part in (4, 8)] + [("lw_split.hip", part, deps_split) for part in (4, 8)]
    extra = os.environ.get("GEOSRAD_HIPCC_FLAGS", "").split()            # kernel experiments (A/B builds) only
    jobs, objs = [], []
    for src, part, deps in units:
        obj = os.path.join(objdir, f"{src[:-4]}_part{part}.o")
        objs.append(obj)
        if force or not os.path.exists(obj) or any(os.path.getmtime(obj) < os.path.getmtime(d) for d in deps):
            jobs.append(subprocess.Popen([hipcc, *flags, *extra, f"-DGEOSRAD_PART={part}", "-c", os.path.join(CSRC, src), "-o", obj]))
    for pr in jobs:
        if pr.wait() != 0:
            raise subprocess.CalledProcessError(pr.returncode, pr.args)
    if jobs or not os.path.exists(SO) or any(os.path.getmtime(SO) < os.path.getmtime(o) for o in objs):
        subprocess.check_call([hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", *objs, "-o", SO])
    return SO


_CTYPES = {"int": ctypes.c_int, "int32_t": ctypes.c_int, "uint64_t": ctypes.c_uint64, "double": ctypes.c_double, "size_t": ctypes.c_size_t}


def parse_header(text):
    """{name: (restype, [(ctype, parameter name), ...])} of every `type geosrad_x(args);` in the text of include/geosrad.h.  A pointer or
    array is c_void_p (`const char *`: c_char_p), the rest as _CTYPES says; a parameter without a name or of another type raises TypeError."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*|^[ \t]*#[^\n]*", "", text, flags=re.S | re.M)            # comments, preprocessor lines

    def ctype(fn, decl):            # decl: a type with its `*` and `[n]`, without the name
        decl = " ".join(decl.replace("*", " * ").split())
        if "*" in decl or "[" in decl:
            return ctypes.c_char_p if decl == "const char *" else ctypes.c_void_p
        if decl not in _CTYPES:
            raise TypeError(f"{fn}: no ctypes type for `{decl}`")
        return _CTYPES[decl]

    protos = {}
    for ret, fn, args in re.findall(r"([\w \t*]+?)\b(geosrad_\w+)\s*\(([^;{}()]*)\)\s*;", text):
        params = []
        for arg in args.split(","):
            m = re.fullmatch(r"(.*[\s*])(\w+)\s*((?:\[\w*\])?)\s*", arg, flags=re.S)
            if not m or not m.group(1).strip():
                raise TypeError(f"{fn}: parameter `{arg.strip()}` has no name")
            params.append((ctype(fn, m.group(1) + m.group(3)), m.group(2)))
        protos[fn] = (ctype(fn, ret), params)
    return protos


@functools.lru_cache(maxsize=None)
def prototypes():
    """parse_header of include/geosrad.h, read once; its names are those of EXPORTS"""
    if not os.path.exists(HEADER):
        raise RuntimeError(f"{HEADER} is missing: the binding takes every entry point's argument order and types from it")
    protos = parse_header(open(HEADER).read())
    if set(protos) != set(EXPORTS):
        raise RuntimeError(f"{HEADER} and _lib.EXPORTS differ: {sorted(set(protos) ^ set(EXPORTS))}")
    return protos


@functools.lru_cache(maxsize=None)
def all_prototypes():
    """prototypes() plus the prototypes of every further header of HEADERS, each held to its own export list"""
    protos = dict(prototypes())
    for path, exports in HEADERS[1:]:
        if not os.path.exists(path):
            raise RuntimeError(f"{path} is missing: the binding takes every entry point's argument order and types from it")
        more = parse_header(open(path).read())
        if set(more) != set(exports):
            raise RuntimeError(f"{path} and its export list differ: {sorted(set(more) ^ set(exports))}")
        protos.update(more)
    return protos


@functools.lru_cache(maxsize=None)
def satsim_prototypes():
    """the prototypes of include/geosrad_satsim.h, held to EXPORTS_SATSIM"""
    if not os.path.exists(HEADER_SATSIM):
        raise RuntimeError(f"{HEADER_SATSIM} is missing: the binding takes every entry point's argument order and types from it")
    protos = parse_header(open(HEADER_SATSIM).read())
    if set(protos) != set(EXPORTS_SATSIM):
        raise RuntimeError(f"{HEADER_SATSIM} and its export list differ: {sorted(set(protos) ^ set(EXPORTS_SATSIM))}")
    return protos


@functools.lru_cache(maxsize=None)
def misr_modis_prototypes():
    """the prototypes of include/geosrad_misr_modis.h, held to EXPORTS_MISR_MODIS"""
    if not os.path.exists(HEADER_MISR_MODIS):
        raise RuntimeError(f"{HEADER_MISR_MODIS} is missing: the binding takes every entry point's argument order and types from it")
    protos = parse_header(open(HEADER_MISR_MODIS).read())
    if set(protos) != set(EXPORTS_MISR_MODIS):
        raise RuntimeError(f"{HEADER_MISR_MODIS} and its export list differ: {sorted(set(protos) ^ set(EXPORTS_MISR_MODIS))}")
    return protos


@functools.lru_cache(maxsize=None)
def lidar_prototypes():
    """the prototypes of include/geosrad_lidar.h, held to EXPORTS_LIDAR"""
    if not os.path.exists(HEADER_LIDAR):
        raise RuntimeError(f"{HEADER_LIDAR} is missing: the binding takes every entry point's argument order and types from it")
    protos = parse_header(open(HEADER_LIDAR).read())
    if set(protos) != set(EXPORTS_LIDAR):
        raise RuntimeError(f"{HEADER_LIDAR} and its export list differ: {sorted(set(protos) ^ set(EXPORTS_LIDAR))}")
    return protos


@functools.lru_cache(maxsize=None)
def radar_prototypes():
    """the prototypes of include/geosrad_radar.h, held to EXPORTS_RADAR"""
    if not os.path.exists(HEADER_RADAR):
        raise RuntimeError(f"{HEADER_RADAR} is missing: the binding takes every entry point's argument order and types from it")
    protos = parse_header(open(HEADER_RADAR).read())
    if set(protos) != set(EXPORTS_RADAR):
        raise RuntimeError(f"{HEADER_RADAR} and its export list differ: {sorted(set(protos) ^ set(EXPORTS_RADAR))}")
    return protos


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(SO):
            raise RuntimeError(f"{SO} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                               "(there is no CPU fallback)")
        protos = {**all_prototypes(), **satsim_prototypes(), **misr_modis_prototypes(), **lidar_prototypes(), **radar_prototypes()}
        # PyTorch ships its own copy of the HIP runtime; when it is going to be used in this process (device tensors and streams
        # handed to the `_dev` entry points) it has to be the one this library binds to, so it is loaded first.
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        L = ctypes.CDLL(SO)
        for name, (restype, params) in protos.items():
            fn = getattr(L, name)
            fn.restype, fn.argtypes = restype, [t for t, _ in params]
        _lib = L
    return _lib
