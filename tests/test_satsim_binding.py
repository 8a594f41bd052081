"""CPU: what the Context methods for include/geosrad_satsim.h hand the C library.  As in tests/test_gettau_binding.py the header is parsed
here (not with the package's parser) and a stub library is built from that parse: one ctypes.CFUNCTYPE of each prototype around a Python
callback that records its arguments.  No device is opened."""
import ctypes
import os
import re

import numpy as np
import pytest

from tests.conftest import ROOT
from geosradiation_gridcomp_amd import _lib, api

HDR = os.path.join(ROOT, "include", "geosrad_satsim.h")
NP, NLEV, NCOL = 5, 4, 3
HANDLE, STREAM = 0x7000, 0x5000
CTYPES = {"int": ctypes.c_int, "double": ctypes.c_double}
OUT = list(api.Context.ICARUS_OUT)


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
    assert sorted(PROTOS) == sorted(_lib.EXPORTS_SATSIM)
    for name, params in PROTOS.items():
        assert [p for p, _ in api._params(name)] == [p for _, p in params], name
        assert [conv for _, conv in api._params(name)] == [{"int": int, "double": float}.get(t) for t, _ in params], name
    assert api._params("geosrad_getirtau_dev")[2][0] == "ib"          # the other headers still answer


def _inputs(ctx, rng):
    r = lambda *s: np.ascontiguousarray(rng.uniform(0.1, 1.0, s), dtype=ctx.dtype)
    d = {k: r(NLEV, NP) for k in ("pfull", "qv", "cc", "conv", "dtau_s", "dtau_c", "at", "dem_s", "dem_c")}
    d.update(phalf=r(NLEV + 1, NP), skt=r(NP), frac_out=r(NLEV, NCOL, NP))
    return d


def test_host_methods(ctx, stub):
    d = _inputs(ctx, np.random.default_rng(2))
    seed = np.arange(NP, dtype=np.int32)
    frac, after = ctx.scops(NP, NLEV, NCOL, seed, d["cc"], d["conv"], 3)
    assert frac.shape == (NLEV, NCOL, NP) and frac.dtype == ctx.dtype and after.dtype == np.int32 and after is not seed
    expect(stub, "geosrad_scops", {"npoints": NP, "nlev": NLEV, "ncol": NCOL, "seed": addr(after), "cc": addr(d["cc"]), "conv": addr(d["conv"]),
                                   "overlap": 3, "frac_out": addr(frac)})
    sunlit = np.ones(NP, np.int32)
    args = (NP, sunlit, NLEV, NCOL, d["pfull"], d["phalf"], d["qv"], d["cc"], d["conv"], d["dtau_s"], d["dtau_c"], 1, 2, 3, d["frac_out"], d["skt"], 0.999,
            d["at"], d["dem_s"], d["dem_c"])
    o = ctx.icarus(*args)
    assert list(o) == OUT and o["fq_isccp"].shape == (7, 7, NP) and o["boxptop"].shape == (NCOL, NP) and o["meantb"].shape == (NP,)
    assert all(v.dtype == ctx.dtype for v in o.values())
    ins = {k: addr(v) for k, v in d.items()}
    scal = {"npoints": NP, "nlev": NLEV, "ncol": NCOL, "top_height": 1, "top_height_direction": 2, "overlap": 3, "emsfc_lw": 0.999, "sunlit": addr(sunlit)}
    expect(stub, "geosrad_icarus", {**scal, **ins, **{k: addr(v) for k, v in o.items()}})
    o = ctx.icarus(*args, want=("boxtau", "meantbclr"))
    assert set(o) == {"boxtau", "meantbclr"}
    expect(stub, "geosrad_icarus", {**scal, **ins, **{k: None for k in OUT}, "boxtau": addr(o["boxtau"]), "meantbclr": addr(o["meantbclr"])})
    # an input of another dtype is converted: what arrives is not the caller's array; sunlit of another integer kind too
    other = np.float64 if ctx.dtype == np.float32 else np.float32
    a2 = list(args); a2[4] = d["pfull"].astype(other); a2[1] = np.ones(NP, np.int64)
    ctx.icarus(*a2)
    a = stub.last("geosrad_icarus")
    assert a["pfull"] not in (None, addr(d["pfull"])) and a["phalf"] == addr(d["phalf"]) and a["sunlit"] not in (None, addr(a2[1]))
    with pytest.raises(TypeError, match="sgfcld"):
        ctx.icarus(*args, want=("sgfcld",))


def test_dev_methods(ctx, stub):
    names = ["seed", "cc", "conv", "frac_out_u8", "sunlit", "pfull", "phalf", "qv", "dtau_s", "dtau_c", "skt", "at", "dem_s", "dem_c", "psfc"] + OUT
    ptr = {k: 0x100000 + 0x100 * i for i, k in enumerate(names)}
    pick = lambda *ks: {k: ptr[k] for k in ks}
    ctx.scops_dev(STREAM, NP, NLEV, NCOL, ptr, 2)
    expect(stub, "geosrad_scops_dev", {"stream": STREAM, "npoints": NP, "nlev": NLEV, "ncol": NCOL, "overlap": 2, **pick("seed", "cc", "conv", "frac_out_u8")})
    ctx.icarus_dev(STREAM, NP, NLEV, NCOL, {k: v for k, v in ptr.items() if k not in ("fq_isccp", "boxtau")}, 3, 1, 2, 0.98)
    expect(stub, "geosrad_icarus_dev", {"stream": STREAM, "npoints": NP, "nlev": NLEV, "ncol": NCOL, "top_height": 3, "top_height_direction": 1, "overlap": 2,
                                        "emsfc_lw": 0.98, **pick(*names[1:14]), **pick(*OUT), "fq_isccp": None, "boxtau": None})
    ctx.cosp_seeds_dev(STREAM, NP, ptr)
    expect(stub, "geosrad_cosp_seeds_dev", {"stream": STREAM, "npoints": NP, **pick("psfc", "seed")})
    fields = ["T", "QV", "FCLD", "CCA", "PLE", "PLO", "DTAU_S", "EMISS", "DTAU_C", "DEM_C", "TS", "SGFCLD"]
    p = {k: 0x200000 + 0x100 * i for i, k in enumerate(fields + ["sunlit", "seed"] + OUT)}
    ctx.isccp_dev(STREAM, NP, NLEV, NCOL, p)          # the GEOS settings are the defaults (GEOS_SatsimGridComp.F90:3360-3362, :3462)
    expect(stub, "geosrad_isccp_dev", {"stream": STREAM, "npoints": NP, "lm": NLEV, "ncol": NCOL, "overlap": 3, "top_height": 1, "top_height_direction": 2,
                                       "emsfc_lw": 0.999, **{k.lower(): p[k] for k in fields}, **{k: p[k] for k in ["sunlit", "seed"] + OUT}})
    q = {k: v for k, v in p.items() if k not in ("CCA", "DTAU_C", "DEM_C", "SGFCLD", "meantb")}
    ctx.isccp_dev(STREAM, NP, NLEV, NCOL, q, overlap=1, top_height=3, top_height_direction=1, emsfc_lw=1.0)
    expect(stub, "geosrad_isccp_dev", {"stream": STREAM, "npoints": NP, "lm": NLEV, "ncol": NCOL, "overlap": 1, "top_height": 3, "top_height_direction": 1,
                                       "emsfc_lw": 1.0, **{k.lower(): q.get(k) for k in fields}, **{k: q.get(k) for k in ["sunlit", "seed"] + OUT}})


def test_every_entry_point_was_called(stub):
    """runs last in this file: every prototype of the header is reached by a Context method"""
    assert {c[0] for c in stub.calls} == set(PROTOS)
