"""CPU: the second public header, include/geosrad_gettau.h, and what the Context methods for it hand the C library.

As in tests/test_api_binding.py the header is parsed here (not with the package's parser) and a stub library is built from that parse: one
ctypes.CFUNCTYPE of each prototype around a Python callback that records its arguments.  No device is opened."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from tests.conftest import ROOT
from geosradiation_gridcomp_amd import _lib, api

HDR = os.path.join(ROOT, "include", "geosrad_gettau.h")
HDR_MAIN = os.path.join(ROOT, "include", "geosrad.h")
NCOL, NLEVS = 3, 5
HANDLE, STREAM = 0x7000, 0x5000
CTYPES = {"int": ctypes.c_int, "int32_t": ctypes.c_int, "uint64_t": ctypes.c_uint64, "double": ctypes.c_double, "size_t": ctypes.c_size_t,
          "const char *": ctypes.c_char_p}
NAMES = ["geosrad_getvistau", "geosrad_getvistau_dev", "geosrad_getnirtau", "geosrad_getnirtau_dev", "geosrad_getirtau", "geosrad_getirtau_dev",
         "geosrad_lw_cloud_diag_dev"]


def parse(text):
    """{name: (return type, [(type, parameter)])}; a pointer or array parameter has the type "*" """
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    text = "\n".join(ln for ln in text.splitlines() if not ln.lstrip().startswith("#"))
    protos = {}
    for ret, name, args in re.findall(r"([\w \t*]+?)\b(geosrad_\w+)\s*\(([^;{}()]*)\)\s*;", text):
        params = []
        for a in args.split(","):
            base, p, arr = re.fullmatch(r"\s*(.*?)(\w+)\s*(\[\w*\])?\s*", a).groups()
            base = " ".join(base.replace("*", " * ").split())
            params.append((base if base == "const char *" or not ("*" in base or arr) else "*", p))
        protos[name] = (" ".join(ret.replace("*", " * ").split()), params)
    return protos


PROTOS = parse(open(HDR).read())


class Stub:
    def __init__(self):
        self.calls, self._keep = [], []
        for name, (ret, params) in PROTOS.items():
            argtypes = [CTYPES.get(t, ctypes.c_void_p) for t, _ in params]
            fn = ctypes.CFUNCTYPE(CTYPES[ret], *argtypes)(self._callback(name, [p for _, p in params]))
            self._keep.append(fn)
            setattr(self, name, fn)

    def _callback(self, name, pnames):
        def cb(*args):
            self.calls.append((name, dict(zip(pnames, args))))
            return 0
        return cb

    def last(self, name):
        got = [c for c in self.calls if c[0] == name]
        assert got, f"{name} was not called"
        return got[-1][1]


@pytest.fixture(scope="module")
def stub():
    return Stub()


@pytest.fixture(params=[4, 8])
def ctx(request, stub):
    c = object.__new__(api.Context)
    c.L, c.h, c.real_kind = stub, ctypes.c_void_p(HANDLE), request.param
    c.dtype = np.float32 if request.param == 4 else np.float64
    yield c
    c.h = ctypes.c_void_p()


def expect(stub, name, want):
    """every parameter of the prototype but ctx is in `want`: a value, or a callable applied to what arrived"""
    a = stub.last(name)
    assert a["ctx"] == HANDLE
    for _, p in PROTOS[name][1]:
        if p == "ctx":
            continue
        assert p in want, f"{name}: the test says nothing about `{p}`"
        assert want[p](a[p]) if callable(want[p]) else a[p] == want[p], (name, p, a[p], want[p])


def addr(x):
    return None if x is None else x.ctypes.data


def test_header_declares_the_gettau_entry_points():
    assert sorted(PROTOS) == sorted(NAMES) == sorted(_lib.EXPORTS_GETTAU)
    assert {t for _, ps in PROTOS.values() for t, _ in ps} == {"*", "int", "double"}
    assert all(ret == "int" and ps[0] == ("*", "ctx") for ret, ps in PROTOS.values())
    for name in NAMES:
        if name.endswith("_dev"):
            assert PROTOS[name][1][1] == ("*", "stream"), name
            host = name[:-4]
            if host in PROTOS:          # the host variant: the same arguments without the stream
                assert PROTOS[host][1] == [PROTOS[name][1][0]] + PROTOS[name][1][2:], name
    # the orders the issue and gettau.F90 state
    order = lambda n: [p for _, p in PROTOS[n][1]]
    assert order("geosrad_getvistau_dev") == ["ctx", "stream", "ncol", "nlevs", "cosz", "dp", "fcld", "reff", "hydromets", "ict", "icb", "grav",
                                              "taubeam", "taudiff", "asycl"]
    assert order("geosrad_getnirtau_dev") == ["ctx", "stream", "ib", "ncol", "nlevs", "cosz", "dp", "fcld", "reff", "hydromets", "ict", "icb", "grav",
                                              "taubeam", "taudiff", "asycl", "ssacl"]
    assert order("geosrad_getirtau_dev") == ["ctx", "stream", "ib", "ncol", "nlevs", "dp", "fcld", "reff", "hydromets", "grav", "taudiag", "tcldlyr", "enn"]
    assert order("geosrad_lw_cloud_diag_dev") == ["ctx", "stream", "ncol", "lm", "grav", "undef", "taucrit", "ple", "t", "fcld", "qi", "ql", "qr", "qs",
                                                  "ri", "rl", "rr", "rs", "tauir", "cldtmp", "cldprs"]
    # every declaration cites the reference lines it replaces
    text = open(HDR).read()
    for cite in ("gettau.F90:33-34", "gettau.F90:102-103", "gettau.F90:173-174", "GEOS_IrradGridComp.F90:1516"):
        assert cite in text, cite


def test_main_header_is_unchanged_in_what_it_declares():
    main = parse(open(HDR_MAIN).read())
    assert len(main) == 75 and set(main) == set(_lib.EXPORTS) and not set(main) & set(PROTOS)
    assert set(_lib.prototypes()) == set(_lib.EXPORTS)
    assert set(_lib.all_prototypes()) == set(_lib.EXPORTS) | set(NAMES)
    assert [h for h, _ in _lib.HEADERS] == [HDR_MAIN, HDR] and _lib.HEADERS[0][1] is _lib.EXPORTS


def test_header_compiles_as_c_and_includes_the_main_one(tmp_path):
    src = tmp_path / "use.c"
    src.write_text('#include "geosrad_gettau.h"\nint (*fn)(geosrad_ctx *, void *, int, int, int, const void *, const void *, const void *, '
                   'const void *, double, void *, void *, void *) = geosrad_getirtau_dev;\n'
                   'int main(void) { geosrad_ctx *c = 0; return GEOSRAD_OK + (c != 0) + (fn == 0); }\n')
    subprocess.check_call([os.environ.get("CC", "cc"), "-Wall", "-Werror", "-I", os.path.dirname(HDR), "-c", str(src), "-o", str(tmp_path / "use.o")])


def test_lib_declares_and_exports_every_prototype():
    L = _lib.lib()
    for name, (ret, params) in PROTOS.items():
        fn = getattr(L, name)                   # libgeosrad.so exports it
        assert fn.restype is ctypes.c_int, name
        assert list(fn.argtypes) == [CTYPES.get(t, ctypes.c_void_p) for t, _ in params], name
        assert [p for _, p in _lib.all_prototypes()[name][1]] == [p for _, p in params]
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.SO], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (geosrad_\w+)", nm))
    assert set(NAMES) <= exported and set(_lib.EXPORTS) <= exported
    # a null context is refused before anything else is looked at
    assert L.geosrad_getvistau_dev(None, None, 1, 1, None, None, None, None, None, 0, 0, ctypes.c_double(9.8), None, None, None) == 1
    assert L.geosrad_lw_cloud_diag_dev(None, None, 1, 1, ctypes.c_double(9.8), ctypes.c_double(1e15), ctypes.c_double(0.3), *([None] * 14)) == 1


def _inputs(ctx, rng):
    r = lambda *s: np.ascontiguousarray(rng.uniform(0.1, 1.0, s), dtype=ctx.dtype)
    return {"cosz": r(NCOL), "dp": r(NLEVS, NCOL), "fcld": r(NLEVS, NCOL), "reff": r(4, NLEVS, NCOL), "hydromets": r(4, NLEVS, NCOL)}


def test_host_methods(ctx, stub):
    d = _inputs(ctx, np.random.default_rng(1))
    ins = {k: addr(v) for k, v in d.items()}
    o = ctx.getvistau(NCOL, NLEVS, d["cosz"], d["dp"], d["fcld"], d["reff"], d["hydromets"], 2, 4)
    assert set(o) == {"taubeam", "taudiff", "asycl"} and o["taubeam"].shape == (4, NLEVS, NCOL) and o["asycl"].shape == (NLEVS, NCOL)
    assert all(v.dtype == ctx.dtype for v in o.values())
    expect(stub, "geosrad_getvistau", {"ncol": NCOL, "nlevs": NLEVS, "ict": 2, "icb": 4, "grav": 9.80665, **ins, **{k: addr(v) for k, v in o.items()}})
    o = ctx.getvistau(NCOL, NLEVS, d["cosz"], d["dp"], d["fcld"], d["reff"], d["hydromets"], 0, 0, grav=9.5, want=("taudiff",))
    assert set(o) == {"taudiff"}
    expect(stub, "geosrad_getvistau", {"ncol": NCOL, "nlevs": NLEVS, "ict": 0, "icb": 0, "grav": 9.5, **ins, "taubeam": None,
                                       "taudiff": addr(o["taudiff"]), "asycl": None})
    o = ctx.getnirtau(3, NCOL, NLEVS, d["cosz"], d["dp"], d["fcld"], d["reff"], d["hydromets"], 2, 4)
    assert set(o) == {"taubeam", "taudiff", "asycl", "ssacl"} and o["ssacl"].shape == (NLEVS, NCOL)
    expect(stub, "geosrad_getnirtau", {"ib": 3, "ncol": NCOL, "nlevs": NLEVS, "ict": 2, "icb": 4, "grav": 9.80665, **ins,
                                       **{k: addr(v) for k, v in o.items()}})
    o = ctx.getirtau(10, NCOL, NLEVS, d["dp"], d["fcld"], d["reff"], d["hydromets"])
    assert set(o) == {"taudiag", "tcldlyr", "enn"} and o["taudiag"].shape == (4, NLEVS, NCOL) and o["enn"].shape == (NLEVS + 1, NCOL)
    del ins["cosz"]
    expect(stub, "geosrad_getirtau", {"ib": 10, "ncol": NCOL, "nlevs": NLEVS, "grav": 9.80665, **ins, **{k: addr(v) for k, v in o.items()}})
    o = ctx.getirtau(1, NCOL, NLEVS, d["dp"], d["fcld"], d["reff"], d["hydromets"], want=["enn"])
    expect(stub, "geosrad_getirtau", {"ib": 1, "ncol": NCOL, "nlevs": NLEVS, "grav": 9.80665, **ins, "taudiag": None, "tcldlyr": None, "enn": addr(o["enn"])})
    # an input of another dtype is converted: what arrives is not the caller's array
    other = np.float64 if ctx.dtype == np.float32 else np.float32
    ctx.getirtau(1, NCOL, NLEVS, d["dp"].astype(other), d["fcld"], d["reff"], d["hydromets"])
    a = stub.last("geosrad_getirtau")
    assert a["dp"] not in (None, addr(d["dp"])) and a["fcld"] == addr(d["fcld"])
    with pytest.raises(TypeError, match="ssacl"):
        ctx.getvistau(NCOL, NLEVS, d["cosz"], d["dp"], d["fcld"], d["reff"], d["hydromets"], 2, 4, want=("ssacl",))


def test_dev_methods(ctx, stub):
    names = ["cosz", "dp", "fcld", "reff", "hydromets", "taubeam", "taudiff", "asycl", "ssacl", "taudiag", "tcldlyr", "enn"]
    ptr = {k: 0x100000 + 0x100 * i for i, k in enumerate(names)}
    pick = lambda *ks: {k: ptr[k] for k in ks}
    ctx.getvistau_dev(STREAM, NCOL, NLEVS, ptr, 2, 4)
    expect(stub, "geosrad_getvistau_dev", {"stream": STREAM, "ncol": NCOL, "nlevs": NLEVS, "ict": 2, "icb": 4, "grav": 9.80665,
                                           **pick("cosz", "dp", "fcld", "reff", "hydromets", "taubeam", "taudiff", "asycl")})
    ctx.getnirtau_dev(STREAM, 2, NCOL, NLEVS, {k: v for k, v in ptr.items() if k not in ("taubeam", "cosz")}, 0, 0, grav=9.5)
    expect(stub, "geosrad_getnirtau_dev", {"stream": STREAM, "ib": 2, "ncol": NCOL, "nlevs": NLEVS, "ict": 0, "icb": 0, "grav": 9.5, "cosz": None,
                                           "taubeam": None, **pick("dp", "fcld", "reff", "hydromets", "taudiff", "asycl", "ssacl")})
    ctx.getirtau_dev(STREAM, 4, NCOL, NLEVS, {k: v for k, v in ptr.items() if k != "tcldlyr"})
    expect(stub, "geosrad_getirtau_dev", {"stream": STREAM, "ib": 4, "ncol": NCOL, "nlevs": NLEVS, "grav": 9.80665, "tcldlyr": None,
                                          **pick("dp", "fcld", "reff", "hydromets", "taudiag", "enn")})
    fields = ["PLE", "T", "FCLD", "QI", "QL", "QR", "QS", "RI", "RL", "RR", "RS", "TAUIR", "CLDTMP", "CLDPRS"]
    p = {k: 0x200000 + 0x100 * i for i, k in enumerate(fields)}
    ctx.lw_cloud_diag_dev(STREAM, NCOL, NLEVS, p)
    expect(stub, "geosrad_lw_cloud_diag_dev", {"stream": STREAM, "ncol": NCOL, "lm": NLEVS, "grav": 9.80665, "undef": 1e15, "taucrit": 0.30,
                                               **{k.lower(): v for k, v in p.items()}})
    ctx.lw_cloud_diag_dev(STREAM, NCOL, NLEVS, {k: v for k, v in p.items() if k not in ("FCLD", "TAUIR")}, taucrit=0.1, grav=9.5, undef=-999.0)
    expect(stub, "geosrad_lw_cloud_diag_dev", {"stream": STREAM, "ncol": NCOL, "lm": NLEVS, "grav": 9.5, "undef": -999.0, "taucrit": 0.1,
                                               **{k.lower(): v for k, v in p.items()}, "fcld": None, "tauir": None})


def test_every_gettau_entry_point_was_called(stub):
    """runs last in this file: every prototype of the header is reached by a Context method"""
    assert {c[0] for c in stub.calls} == set(NAMES)
