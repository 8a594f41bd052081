"""CPU: what the Context methods for include/geosrad_misr_modis.h hand the C library.  As in tests/test_satsim_binding.py the header is
parsed here (not with the package's parser) and a stub library is built from that parse: one ctypes.CFUNCTYPE of each prototype around a
Python callback that records its arguments.  No device is opened."""
import ctypes
import os
import re

import numpy as np
import pytest

from tests.conftest import ROOT
from geosradiation_gridcomp_amd import _lib, api

HDR = os.path.join(ROOT, "include", "geosrad_misr_modis.h")
NP, NLEV, NCOL = 5, 4, 3
HANDLE, STREAM = 0x7000, 0x5000
CTYPES = {"int": ctypes.c_int, "double": ctypes.c_double}
OUT = list(api.Context.MISR_OUT)


def parse(text):
    """{name: [(type, parameter)]}; a pointer parameter has the type "*" """
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    text = "\n".join(ln for ln in text.splitlines() if not ln.lstrip().startswith("#"))
    protos = {}
    for ret, name, args in re.findall(r"([\w \t*]+?)\b(geosrad_\w+)\s*\(([^;{}()]*)\)\s*;", text):
        assert ret.strip() == "int", name
        params = []
        for a in args.split(","):
            base, p = re.fullmatch(r"\s*(.*?)(\w+)\s*", a, flags=re.S).groups()
            params.append(("*" if "*" in base else base.strip(), p))
        protos[name] = params
    return protos


PROTOS = parse(open(HDR).read())


class Stub:
    def __init__(self):
        self.calls, self._keep = [], []
        for name, params in PROTOS.items():
            fn = ctypes.CFUNCTYPE(ctypes.c_int, *[CTYPES.get(t, ctypes.c_void_p) for t, _ in params])(self._callback(name, [p for _, p in params]))
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
    for _, p in PROTOS[name]:
        if p == "ctx":
            continue
        assert p in want, f"{name}: the test says nothing about `{p}`"
        assert want[p](a[p]) if callable(want[p]) else a[p] == want[p], (name, p, a[p], want[p])


def addr(x):
    return None if x is None else x.ctypes.data


def test_the_binding_reads_its_argument_lists_from_the_header():
    assert sorted(PROTOS) == sorted(_lib.EXPORTS_MISR_MODIS)
    for name, params in PROTOS.items():
        assert [p for p, _ in api._params(name)] == [p for _, p in params], name
        assert [conv for _, conv in api._params(name)] == [{"int": int, "double": float}.get(t) for t, _ in params], name
    # the other three headers still answer
    assert api._params("geosrad_getirtau_dev")[2][0] == "ib" and api._params("geosrad_scops_dev")[5][0] == "seed" and api._params("geosrad_check")[0][0] == "ctx"


def test_host_method(ctx, stub):
    rng = np.random.default_rng(3)
    r = lambda *s: np.ascontiguousarray(rng.uniform(0.1, 1.0, s), dtype=ctx.dtype)
    d = {k: r(NLEV, NP) for k in ("zfull", "at", "dtau_s", "dtau_c")}
    d["frac_out"] = r(NLEV, NCOL, NP)
    sunlit = np.ones(NP, np.int32)
    args = (NP, NLEV, NCOL, sunlit, d["zfull"], d["at"], d["dtau_s"], d["dtau_c"], d["frac_out"], -1.0e30)
    o = ctx.misr(*args)
    assert list(o) == OUT and o["fq_MISR_TAU_v_CTH"].shape == (16, 7, NP) and o["dist_model_layertops"].shape == (16, NP)
    assert o["MISR_mean_ztop"].shape == o["MISR_cldarea"].shape == (NP,) and all(v.dtype == ctx.dtype for v in o.values())
    scal = {"npoints": NP, "nlev": NLEV, "ncol": NCOL, "missing_value": -1.0e30, "sunlit": addr(sunlit)}
    ins = {k: addr(v) for k, v in d.items()}
    expect(stub, "geosrad_misr", {**scal, **ins, **{k: addr(v) for k, v in o.items()}})
    o = ctx.misr(*args, want=("MISR_cldarea",))
    assert set(o) == {"MISR_cldarea"}
    expect(stub, "geosrad_misr", {**scal, **ins, **{k: None for k in OUT}, "MISR_cldarea": addr(o["MISR_cldarea"])})
    # an input of another dtype is converted: what arrives is not the caller's array; sunlit of another integer kind too
    other = np.float64 if ctx.dtype == np.float32 else np.float32
    a2 = list(args); a2[4] = d["zfull"].astype(other); a2[3] = np.ones(NP, np.int64)
    ctx.misr(*a2)
    a = stub.last("geosrad_misr")
    assert a["zfull"] not in (None, addr(d["zfull"])) and a["at"] == addr(d["at"]) and a["sunlit"] not in (None, addr(a2[3]))
    with pytest.raises(TypeError, match="boxtau"):
        ctx.misr(*args, want=("boxtau",))


def test_dev_method(ctx, stub):
    names = ["sunlit", "zfull", "at", "dtau_s", "dtau_c", "frac_out_u8"] + OUT
    ptr = {k: 0x100000 + 0x100 * i for i, k in enumerate(names)}
    ctx.misr_dev(STREAM, NP, NLEV, NCOL, ptr, -1.0e30)
    expect(stub, "geosrad_misr_dev", {"stream": STREAM, "npoints": NP, "nlev": NLEV, "ncol": NCOL, "missing_value": -1.0e30, **ptr})
    ctx.misr_dev(STREAM, NP, NLEV, NCOL, {k: v for k, v in ptr.items() if k not in ("dist_model_layertops", "MISR_mean_ztop")}, 0.0)
    expect(stub, "geosrad_misr_dev", {"stream": STREAM, "npoints": NP, "nlev": NLEV, "ncol": NCOL, "missing_value": 0.0, **ptr,
                                      "dist_model_layertops": None, "MISR_mean_ztop": None})


MODIS_IN = ["t", "p", "dtau_s", "dtau_c", "mr_lsliq", "mr_lsice", "mr_cvliq", "mr_cvice", "reff_lsliq", "reff_lsice", "reff_cvliq", "reff_cvice"]


def test_modis_host_method(ctx, stub):
    rng = np.random.default_rng(4)
    r = lambda *s: np.ascontiguousarray(rng.uniform(0.1, 1.0, s), dtype=ctx.dtype)
    d = {k: r(NLEV, NP) for k in MODIS_IN}
    d.update(ph=r(NLEV + 1, NP), frac_out=r(NLEV, NCOL, NP), isccp_boxtau=r(NCOL, NP), isccp_boxptop=r(NCOL, NP))
    sunlit = np.ones(NP, np.int32)
    order = ["t", "p", "ph", "dtau_s", "dtau_c", "frac_out"] + MODIS_IN[4:] + ["isccp_boxtau", "isccp_boxptop"]
    o = ctx.modis(NP, NLEV, NCOL, sunlit, *[d[k] for k in order])
    assert list(o) == ["modis_mean", "modis_hist"] and o["modis_mean"].shape == (17, NP) and o["modis_hist"].shape == (7, 7, NP)
    scal = {"npoints": NP, "nlev": NLEV, "ncol": NCOL, "sunlit": addr(sunlit)}
    none = {k: None for k in api.Context.MODIS_OUT}
    expect(stub, "geosrad_modis", {**scal, **{k: addr(v) for k, v in d.items()}, **none, **{k: addr(v) for k, v in o.items()}})
    # the optional inputs as None arrive as NULL; the L2 outputs on request, phase as int32
    d2 = dict(d, dtau_c=None, mr_cvliq=None, mr_cvice=None, reff_cvliq=None, reff_cvice=None, isccp_boxtau=None)
    o = ctx.modis(NP, NLEV, NCOL, sunlit, *[d2[k] for k in order], want=api.Context.MODIS_OUT)
    assert list(o) == list(api.Context.MODIS_OUT) and o["phase"].dtype == np.int32 and o["phase"].shape == o["size"].shape == (NCOL, NP)
    assert all(o[k].dtype == ctx.dtype for k in o if k != "phase")
    expect(stub, "geosrad_modis", {**scal, **{k: addr(v) for k, v in d2.items()}, **{k: addr(v) for k, v in o.items()}})
    assert len(api.Context.MODIS_MEAN) == 17
    with pytest.raises(TypeError, match="boxtau"):
        ctx.modis(NP, NLEV, NCOL, sunlit, *[d[k] for k in order], want=("boxtau",))


def test_modis_and_cosp_dev_methods(ctx, stub):
    names = ["sunlit", "t", "p", "ph", "dtau_s", "dtau_c", "frac_out_u8"] + MODIS_IN[4:] + ["isccp_boxtau", "isccp_boxptop"] + list(api.Context.MODIS_OUT)
    ptr = {k: 0x300000 + 0x100 * i for i, k in enumerate(names)}
    ctx.modis_dev(STREAM, NP, NLEV, NCOL, ptr)
    expect(stub, "geosrad_modis_dev", {"stream": STREAM, "npoints": NP, "nlev": NLEV, "ncol": NCOL, **ptr})
    q = {k: v for k, v in ptr.items() if k not in ("dtau_c", "mr_cvliq", "reff_cvice", "phase", "modis_hist")}
    ctx.modis_dev(STREAM, NP, NLEV, NCOL, q)
    expect(stub, "geosrad_modis_dev", {"stream": STREAM, "npoints": NP, "nlev": NLEV, "ncol": NCOL, **{k: q.get(k) for k in ptr}})
    fields = ["T", "QV", "FCLD", "CCA", "PLE", "PLO", "DTAU_S", "EMISS", "DTAU_C", "DEM_C", "TS", "SGFCLD", "ZLE", "QLTOT", "QITOT", "RDFL", "RDFI"]
    outs = list(api.Context.ICARUS_OUT) + OUT + ["modis_mean", "modis_hist"]
    p = {k: 0x400000 + 0x100 * i for i, k in enumerate(fields + ["sunlit", "seed"] + outs)}
    ctx.cosp_dev(STREAM, NP, NLEV, NCOL, p)          # the GEOS settings are the defaults, as for isccp_dev
    expect(stub, "geosrad_cosp_dev", {"stream": STREAM, "npoints": NP, "lm": NLEV, "ncol": NCOL, "overlap": 3, "top_height": 1, "top_height_direction": 2,
                                      "emsfc_lw": 0.999, **{k.lower(): p[k] for k in fields}, **{k: p[k] for k in ["sunlit", "seed"] + outs}})
    q = {k: v for k, v in p.items() if k not in ("CCA", "DTAU_C", "DEM_C", "SGFCLD") + tuple(OUT)}
    ctx.cosp_dev(STREAM, NP, NLEV, NCOL, q, overlap=1, top_height=3, top_height_direction=1, emsfc_lw=1.0)
    expect(stub, "geosrad_cosp_dev", {"stream": STREAM, "npoints": NP, "lm": NLEV, "ncol": NCOL, "overlap": 1, "top_height": 3, "top_height_direction": 1,
                                      "emsfc_lw": 1.0, **{k.lower(): q.get(k) for k in fields}, **{k: q.get(k) for k in ["sunlit", "seed"] + outs}})


def test_every_entry_point_was_called(stub):
    """runs last in this file: every prototype of the header is reached by a Context method"""
    assert {c[0] for c in stub.calls} == set(PROTOS)
