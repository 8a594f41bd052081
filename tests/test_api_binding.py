"""CPU: what every Context method hands the C library, checked against include/geosrad.h by parameter name.

The header is parsed here (not with the package's parser) and a stub library is built from it: one ctypes.CFUNCTYPE of each prototype around
a Python callback that records its arguments, so every call goes through ctypes' own conversion and a wrong count or kind fails here.  No
device is opened: the Context is made without __init__, its handle is a made-up number and device "addresses" are made-up integers."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from tests.conftest import ROOT
from geosradiation_gridcomp_amd import _lib, api, gridcomp as G

HDR = os.path.join(ROOT, "include", "geosrad.h")
NCOL, NLAY, NSUB, NRATS, NBAER, NLIT = 3, 4, 2, 2, 2, 2
HANDLE, STREAM = 0x7000, 0x5000
CTYPES = {"int": ctypes.c_int, "int32_t": ctypes.c_int, "uint64_t": ctypes.c_uint64, "double": ctypes.c_double, "size_t": ctypes.c_size_t,
          "const char *": ctypes.c_char_p}
FIXED = {"geosrad_workspace_bytes": 4096, "geosrad_get_overcast": 3, "geosrad_kernel_label": b"k_stub"}
# pointer-table parameters: entry point family -> {parameter: (gridcomp list, header counter)}
TABLES = {
    "lw_driver_rrtmg": {"in": ("LWD_IN", "LWD_NIN"), "out": ("LWD_OUT", "LWD_NOUT"), "rat_out": ("LWD_RAT_OUT", "LWD_NRATOUT"),
                        "na_out": ("LWNA_OUT", "LWNA_NOUT")},
    "lw_chou_post": {"in": ("LWC_IN", "LWC_NIN"), "out": ("LWC_OUT", "LWC_NOUT")},
    "lw_driver_chou": {"in": ("LWK_IN", "LWK_NIN"), "out": ("LWK_OUT", "LWK_NOUT")},
    "sw_driver_rrtmg": {"in": ("SWD_IN", "SWD_NIN"), "out": ("SWD_OUT", "SWD_NOUT")},
    "sw_driver_chou": {"in": ("SWC_IN", "SWC_NIN"), "out": ("SWC_OUT", "SWC_NOUT"), "na_out": ("SWCNA_OUT", "SWCNA_NOUT")},
    "lw_update_flx": {"in": ("LWU_IN", "LWU_NIN"), "out": ("LWU_OUT", "LWU_NOUT")},
    "lw_update_rats": {"in": ("LWR_IN", "LWR_NIN"), "out": ("LWR_OUT", "LWR_NOUT")},
    "sw_update_export": {"in": ("SWU_IN", "SWU_NIN"), "out": ("SWU_OUT", "SWU_NOUT")},
    "sw_update_surface": {"in": ("SWS_IN", "SWS_NIN"), "out": ("SWS_OUT", "SWS_NOUT")},
    "sw_update_clouds": {"in": ("SWK_IN", "SWK_NIN"), "out": ("SWK_OUT", "SWK_NOUT")},
    "sw_update_cldhb": {"in": ("SWHB_IN", "SWHB_NIN"), "out": ("SWHB_OUT", "SWHB_NOUT")},
    "rad_tendencies": {"in": ("RT_IN", "RT_NIN"), "out": ("RT_OUT", "RT_NOUT")},
    "sorad_na": {"na_out": ("SONA_OUT", "SONA_NOUT")},
}
# header parameter -> key of `ptr` / `inp` on the Python side, where they differ
PYKEY = {
    "rrtmg_sw": {"cld": "cldf", "tauaer": "tauaer_sw", "ssaaer": "ssaaer_sw", "asmaer": "asmaer_sw", "clearCounts": "clearCounts_sw"},
    "mcica": {"zmid": "zm", "cldfrac": "cldf"},
    "lw_update_bands": {"tsinst": "TSINST", "ts_int": "TS_INT", "olrb_int": "OLRB", "dolrb_int": "DOLRB", "olrb_exp": "OLRB_EXP",
                        "tbrb_exp": "TBRB_EXP"},
}


def parse(text):
    """{name: (return type, [(type, parameter)])}; a pointer or array parameter has the type "*" (`const char *` keeps its own)"""
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


def family(name):
    return next((f for f in sorted(TABLES, key=len, reverse=True) if name.startswith("geosrad_" + f)), None)


@pytest.fixture(scope="module")
def counters(tmp_path_factory):
    """{counter: value} of the GEOSRAD_*_N* enumerators the tables are sized by, printed by a program that includes the header"""
    tmp = tmp_path_factory.mktemp("counters")
    names = sorted({c for t in TABLES.values() for _, c in t.values()})
    src = tmp / "counters.c"
    src.write_text('#include <stdio.h>\n#include "geosrad.h"\nint main(void) {\n' +
                   "".join(f'    printf("{n} %d\\n", (int)GEOSRAD_{n});\n' for n in names) + "    return 0;\n}\n")
    exe = str(tmp / "counters")
    subprocess.check_call([os.environ.get("CC", "cc"), "-I", os.path.dirname(HDR), str(src), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, check=True).stdout
    return {a: int(b) for a, b in (ln.split() for ln in out.splitlines())}


class Stub:
    """the library as the header declares it; .calls = [(function, {parameter: value as ctypes delivered it}, {parameter: host array read
    back during the call})]"""

    def __init__(self, counters):
        self.calls, self.rc, self._keep = [], {}, []
        for name, (ret, params) in PROTOS.items():
            restype = ctypes.c_void_p if ret == "const char *" else CTYPES[ret]          # a string goes back as the address of a kept buffer
            argtypes = [CTYPES.get(t, ctypes.c_void_p) for t, _ in params]
            fn = ctypes.CFUNCTYPE(restype, *argtypes)(self._callback(name, [p for _, p in params], counters))
            self._keep.append(fn)
            setattr(self, name, (lambda *a, _fn=fn: ctypes.string_at(_fn(*a))) if ret == "const char *" else fn)

    def _callback(self, name, pnames, counters):
        tabs = TABLES.get(family(name), {})

        def read(ctype, addr, n):
            return None if not addr else list(ctypes.cast(addr, ctypes.POINTER(ctype))[:n])

        def cb(*args):
            a = dict(zip(pnames, args))
            mem = {p: read(ctypes.c_void_p, a[p], counters[tabs[p][1]]) for p in tabs if p in a}
            for p, like in (("dark", "out"), ("dark_na", "na_out"), ("dark_obio", None)):
                if p in a:
                    mem[p] = read(ctypes.c_double, a[p], 2 if like is None else counters[tabs[like][1]])
            if "band_output" in a:
                mem["band_output"] = read(ctypes.c_int32, a["band_output"], 16)
            if "rat_gas" in a:
                mem["rat_gas"] = read(ctypes.c_int32, a["rat_gas"], a["nrats"])
            if "seed_order" in a:
                mem["seed_order"] = read(ctypes.c_int32, a["seed_order"], 4)
            for p in ("consts", "wavenum1", "wavenum2", "adl", "rdl", "wvn1", "wvn2"):
                if p in a:
                    mem[p] = read(ctypes.c_double, a[p], {"consts": 2, "adl": 4, "rdl": 4, "wvn1": 2, "wvn2": 2}.get(p, 16))
            for p in ("hk_uv", "hk_ir", "bndscl", "bndsolvar", "indsolvar", "solcycfrac"):       # host reals: the first element, read as either kind
                if p in a:
                    mem[p] = a[p] and (ctypes.cast(a[p], ctypes.POINTER(ctypes.c_float))[0], ctypes.cast(a[p], ctypes.POINTER(ctypes.c_double))[0])
            if name == "geosrad_lit_index_dev" and a["nlit_host"]:
                ctypes.cast(a["nlit_host"], ctypes.POINTER(ctypes.c_int))[0] = NLIT
            if name == "geosrad_profile_read":
                ctypes.cast(a["total_ms"], ctypes.POINTER(ctypes.c_double))[0] = 1.5
                ctypes.cast(a["launches"], ctypes.POINTER(ctypes.c_long))[0] = 7
            if name == "geosrad_create" or name == "geosrad_create_multi":
                ctypes.cast(a["ctx"], ctypes.POINTER(ctypes.c_void_p))[0] = HANDLE
            if name == "geosrad_obio_weights":
                ctypes.cast(a["npairs"], ctypes.POINTER(ctypes.c_int32))[0] = 5
            self.calls.append((name, a, mem))
            ret = FIXED.get(name, self.rc.get(name, 0))
            if isinstance(ret, bytes):
                self._keep.append(ctypes.create_string_buffer(ret))
                ret = ctypes.addressof(self._keep[-1])
            return ret
        return cb

    def last(self, name):
        got = [c for c in self.calls if c[0] == name]
        assert got, f"{name} was not called"
        return got[-1][1], got[-1][2]


@pytest.fixture(scope="module")
def stub(counters):
    return Stub(counters)


@pytest.fixture(params=[4, 8])
def ctx(request, stub):
    c = object.__new__(api.Context)
    c.L, c.h, c.real_kind = stub, ctypes.c_void_p(HANDLE), request.param
    c.dtype = np.float32 if request.param == 4 else np.float64
    yield c
    c.h = ctypes.c_void_p()             # nothing for __del__ to destroy


def fake(names, base):
    """name -> distinct made-up device address"""
    return {k: base + 0x100 * (i + 1) for i, k in enumerate(names)}


def pointers(name):
    return [p for t, p in PROTOS[name][1] if t == "*" and p not in ("ctx", "stream")]


def expect(stub, name, want, tables=None, ptr=None):
    """the last call of `name`: every parameter of the prototype is in `want` (parameter -> value; a callable is applied to what arrived),
    or is a table of `tables` = {parameter: name -> address, or None for NULL}"""
    a, mem = stub.last(name)
    tables = tables or {}
    for t, p in PROTOS[name][1]:
        if p == "ctx" and p not in want:
            assert a[p] == HANDLE, name
            continue
        if p in tables:
            src = tables[p]
            if src is None:
                assert a[p] is None, (name, p)
                continue
            names = getattr(G, TABLES[family(name)][p][0])
            assert mem[p] == [src.get(k) for k in names], (name, p)          # a name left out arrives as NULL; length = the header's counter
            continue
        assert p in want, f"{name}: the test says nothing about `{p}`"
        w = want[p]
        if callable(w):
            assert w(mem.get(p, a[p])), (name, p, a[p])          # a host array: what the callback read from it during the call
        else:
            assert a[p] == w, (name, p, a[p], w)


def reals(ctx, rng, **shapes):
    return {k: np.ascontiguousarray(rng.uniform(0.1, 1.0, s), dtype=ctx.dtype) for k, s in shapes.items()}


def addr(x):
    return None if x is None else x.ctypes.data


# ---------------------------------------------------------------------------------------------------------------------------------
def test_header_parses_to_the_exports():
    assert set(PROTOS) == set(_lib.EXPORTS) and len(PROTOS) == 75
    kinds = {t for _, ps in PROTOS.values() for t, _ in ps}
    assert kinds == {"*", "const char *", "int", "double", "size_t", "uint64_t"}


def test_lib_declares_every_prototype():
    L = _lib.lib()
    for name, (ret, params) in PROTOS.items():
        fn = getattr(L, name)
        assert fn.restype is {"int": ctypes.c_int, "size_t": ctypes.c_size_t, "const char *": ctypes.c_char_p}[ret], name
        assert list(fn.argtypes) == [CTYPES.get(t, ctypes.c_void_p) for t, _ in params], name
        assert [p for _, p in _lib.prototypes()[name][1]] == [p for _, p in params]


def test_context_lifecycle_and_settings(stub, monkeypatch, tmp_path):
    monkeypatch.setattr(_lib, "lib", lambda: stub)
    c = api.Context(8, device=2)
    expect(stub, "geosrad_create", {"ctx": bool, "device_id": 2, "real_kind": 8})
    assert c.h.value == HANDLE and c.L is stub and c.real_kind == 8 and c.dtype is np.float64
    for fn, f in (("lw", "rrtmg_lw"), ("sw", "rrtmg_sw"), ("chou_lw", "chou_lw"), ("chou_sw", "chou_sw")):
        expect(stub, "geosrad_load_tables_" + fn, {"path": os.fsencode(os.path.join(_lib.DATA, f + "_r8.grtb"))})
    c.rrtmg_lw_ini(str(tmp_path / "x.grtb"))
    expect(stub, "geosrad_load_tables_lw", {"path": os.fsencode(str(tmp_path / "x.grtb"))})
    c.set_inhomogeneity(2)
    expect(stub, "geosrad_load_inhomogeneity", {"ih": 2, "path": os.fsencode(os.path.join(_lib.DATA, "xcw_gamma_r8.grtb"))})
    c.unset_inhomogeneity()
    expect(stub, "geosrad_load_inhomogeneity", {"ih": 0, "path": None})
    c.initialize_cloud_subcol_gen(adl=(1., 2., 3., 4.))
    expect(stub, "geosrad_set_corr_lengths", {"adl": bool, "rdl": None})
    assert stub.last("geosrad_set_corr_lengths")[1]["adl"] == [1., 2., 3., 4.]
    c.set_chunk(77)
    expect(stub, "geosrad_set_chunk", {"max_columns": 77})
    assert c.workspace_bytes() == 4096 and stub.last("geosrad_workspace_bytes")[0]["ctx"] == HANDLE
    c.set_overcast(sorad=True)
    expect(stub, "geosrad_set_overcast", {"flags": 2})
    assert c.overcast == {"irrad": True, "sorad": True} and stub.last("geosrad_get_overcast")[0]["ctx"] == HANDLE
    c.profile(True)
    expect(stub, "geosrad_profile", {"enable": 1})
    assert c.profile_read() == {"k_stub": (1.5, 7)}
    expect(stub, "geosrad_profile_read", {"kernel_id": 13, "total_ms": bool, "launches": bool})
    expect(stub, "geosrad_kernel_label", {"kernel_id": 13})
    c.check(STREAM)
    expect(stub, "geosrad_check", {"stream": STREAM})
    # a non-zero return code: the text of geosrad_last_error, the class by the code, the code in .rc
    for rc, cls in ((5, api.GeosradInputError), (3, api.GeosradError)):
        stub.rc["geosrad_check"] = rc
        FIXED["geosrad_last_error"] = b"negative values in input: play"
        try:
            with pytest.raises(cls, match="negative values in input: play") as e:
                c.check()
            assert e.value.rc == rc and stub.last("geosrad_last_error")[0]["ctx"] == HANDLE
        finally:
            del stub.rc["geosrad_check"], FIXED["geosrad_last_error"]
    c.close()
    expect(stub, "geosrad_destroy", {})
    assert not c.h
    c = api.Context(4, devices=[1, 3], tables=False)
    expect(stub, "geosrad_create_multi", {"ctx": bool, "device_ids": bool, "ndev": 2, "real_kind": 4})
    c.close()


def lw_inputs(ctx, rng):
    d = reals(ctx, rng, play=(NLAY, NCOL), plev=(NLAY + 1, NCOL), tlay=(NLAY, NCOL), tlev=(NLAY + 1, NCOL), tsfc=NCOL, emis=(16, NCOL),
              tauaer=(16, NLAY, NCOL), zm=(NLAY, NCOL), alat=NCOL, **{k: (NLAY, NCOL) for k in api._IN2D})
    return d


LW_OUT = ["clearCounts", "uflx", "dflx", "uflxc", "dflxc", "duflx_dTs", "duflxc_dTs", "olrb", "dolrb_dTs"]
LW_NA = ["uflx_na", "dflx_na", "uflxc_na", "dflxc_na", "duflx_dTs_na", "duflxc_dTs_na"]


def test_rrtmg_lw_host(ctx, stub):
    rng = np.random.default_rng(1)
    d = lw_inputs(ctx, rng)
    bo = np.arange(16, dtype=np.int32) % 2
    for meth, fn, outs in ((ctx.rrtmg_lw, "geosrad_rrtmg_lw", LW_OUT), (ctx.rrtmg_lw_na, "geosrad_rrtmg_lw_na", LW_OUT + LW_NA)):
        o = meth(NCOL, NLAY, 9, True, d["play"], d["plev"], d["tlay"], d["tlev"], d["tsfc"], d["emis"], *[d[k] for k in api._IN2D], 3, 1,
                 d["tauaer"], d["zm"], d["alat"], 200, 2, 3, band_output=bo)
        assert set(o) == set(outs) and o["uflx"].shape == (NLAY + 1, NCOL) and o["olrb"].shape == (NCOL, 16)
        assert o["clearCounts"].dtype == np.int32 and o["clearCounts"].shape == (4, NCOL) and o["dflx"].dtype == ctx.dtype
        want = {"ncol": NCOL, "nlay": NLAY, "psize": 9, "dudTs": 1, "iceflglw": 3, "liqflglw": 1, "dyofyr": 200, "cloudLM": 2, "cloudMH": 3,
                "band_output": addr(bo), **{k: addr(v) for k, v in d.items()}, **{k: addr(o[k]) for k in outs}}
        expect(stub, fn, want)
        assert stub.last(fn)[1]["band_output"] == list(bo)
        o2 = meth(NCOL, NLAY, 4, False, d["play"], d["plev"], d["tlay"], d["tlev"], d["tsfc"], d["emis"], *[d[k] for k in api._IN2D], 3, 1,
                  None, d["zm"], d["alat"], 200, 2, 3, out=o)                    # no aerosol, the caller's own output arrays, no band output
        assert o2 is o
        expect(stub, fn, dict(want, psize=4, dudTs=0, tauaer=None, band_output=bool))
        assert stub.last(fn)[1]["band_output"] == [0] * 16
    inp = dict(d, dyofyr=200, cloudLM=2, cloudMH=3)
    o = ctx.rrtmg_lw_columns(inp)
    expect(stub, "geosrad_rrtmg_lw", dict(want, psize=4, band_output=bool, **{k: addr(o[k]) for k in LW_OUT}))
    o = ctx.rrtmg_lw_na_columns(inp, dudTs=False)
    expect(stub, "geosrad_rrtmg_lw_na", dict(want, psize=4, dudTs=0, band_output=bool, **{k: addr(o[k]) for k in LW_OUT + LW_NA}))
    taug, pfr = ctx.rrtmg_lw_taumol(inp)
    assert taug.shape == pfr.shape == (NCOL, 140, NLAY)
    expect(stub, "geosrad_rrtmg_lw_taumol", {"ncol": NCOL, "nlay": NLAY, "taug": addr(taug), "pfracs": addr(pfr),
                                             **{k: addr(d[k]) for k in ["play", "plev", "tlay", "tlev", "tsfc", "emis", "tauaer"] + api._IN2D[:10]}})


def test_inputs_are_passed_contiguous_in_the_context_kind(ctx, stub):
    """an input of another dtype or a strided one is converted: what arrives is not the caller's array"""
    rng = np.random.default_rng(2)
    d = lw_inputs(ctx, rng)
    other = np.float64 if ctx.dtype == np.float32 else np.float32
    d["tlay"] = d["tlay"].astype(other)
    d["play"] = np.asfortranarray(d["play"])
    ctx.rrtmg_lw(NCOL, NLAY, 4, True, d["play"], d["plev"], d["tlay"], d["tlev"], d["tsfc"], d["emis"], *[d[k] for k in api._IN2D], 3, 1,
                 d["tauaer"], d["zm"], d["alat"], 200, 2, 3)
    a, _ = stub.last("geosrad_rrtmg_lw")
    assert a["tlay"] not in (None, addr(d["tlay"])) and a["play"] not in (None, addr(d["play"])) and a["plev"] == addr(d["plev"])


SW_SCAL = {"rpart": 6, "ncol": NCOL, "nlay": NLAY, "scon": 1360.5, "adjes": 1.25, "isolvar": 1, "iceflgsw": 3, "liqflgsw": 1, "dyofyr": 200, "iaer": 10,
           "cloudLM": 2, "cloudMH": 3, "normFlx": 1, "do_drfband": 1}
SW_OUT = ["clearCounts", "swuflx", "swdflx", "swuflxc", "swdflxc", "nirr", "nirf", "parr", "parf", "uvrr", "uvrf", "fswband"] + api._SW_COT


def first(ctx, value):
    """the host real array that arrived starts with `value` in the context's kind"""
    return lambda got: bool(got) and got[0 if ctx.dtype == np.float32 else 1] == ctx.dtype(value)


def sw_inputs(ctx, rng):
    return reals(ctx, rng, coszen=NCOL, play=(NLAY, NCOL), plev=(NLAY + 1, NCOL), tlay=(NLAY, NCOL), cld=(NLAY, NCOL), ciwp=(NLAY, NCOL),
                 clwp=(NLAY, NCOL), rei=(NLAY, NCOL), rel=(NLAY, NCOL), zm=(NLAY, NCOL), alat=NCOL, tauaer=(14, NLAY, NCOL),
                 ssaaer=(14, NLAY, NCOL), asmaer=(14, NLAY, NCOL), asdir=NCOL, asdif=NCOL, aldir=NCOL, aldif=NCOL,
                 **{k: (NLAY, NCOL) for k in api._SW_GAS})


def test_rrtmg_sw_host(ctx, stub):
    rng = np.random.default_rng(3)
    d = sw_inputs(ctx, rng)
    sv = {"bndscl": first(ctx, 0.5), "indsolvar": first(ctx, 0.25), "solcycfrac": first(ctx, 0.75)}
    for meth, fn, outs in ((ctx.rrtmg_sw, "geosrad_rrtmg_sw", SW_OUT + ["drband", "dfband"]),
                           (ctx.rrtmg_sw_radval, "geosrad_rrtmg_sw_radval", SW_OUT + ["drband", "dfband", "radval"])):
        o = meth(6, NCOL, NLAY, 1360.5, 1.25, d["coszen"], 1, d["play"], d["plev"], d["tlay"], *[d[k] for k in api._SW_GAS], 3, 1, d["cld"],
                 d["ciwp"], d["clwp"], d["rei"], d["rel"], 200, d["zm"], d["alat"], 10, d["tauaer"], d["ssaaer"], d["asmaer"], d["asdir"],
                 d["asdif"], d["aldir"], d["aldif"], 2, 3, 1, do_drfband=True, bndscl=[0.5] * 14, indsolvar=[0.25, 1.0], solcycfrac=0.75)
        assert set(outs) <= set(o) and o["swuflx"].shape == (NLAY + 1, NCOL) and o["fswband"].shape == o["drband"].shape == (14, NCOL)
        assert o["nirr"].shape == (NCOL,) and o["clearCounts"].dtype == np.int32 and o["cotdtp"].dtype == ctx.dtype
        expect(stub, fn, {**SW_SCAL, **sv, **{k: addr(v) for k, v in d.items()}, **{k: addr(o[k]) for k in outs}})
        if "radval" in outs:
            assert o["radval"].shape == (120, NCOL) and set(api.RADVAL_NAMES) <= set(o) and np.shares_memory(o["forinlp"], o["radval"][119])
    inp = dict(d, cldf=d["cld"], tauaer_sw=d["tauaer"], ssaaer_sw=d["ssaaer"], asmaer_sw=d["asmaer"], dyofyr=200, cloudLM=2, cloudMH=3)
    o = ctx.rrtmg_sw_columns(inp)                              # defaults: no aerosol, no drband, no solar variability
    none = {k: None for k in ("tauaer", "ssaaer", "asmaer", "drband", "dfband", "bndscl", "indsolvar", "solcycfrac")}
    expect(stub, "geosrad_rrtmg_sw", {**SW_SCAL, "rpart": 4, "scon": 1361.0, "adjes": 1.0, "isolvar": 0, "iaer": 0, "normFlx": 0, "do_drfband": 0,
                                      **{k: addr(v) for k, v in d.items()}, **{k: addr(o[k]) for k in SW_OUT}, **none})
    taug, taur, ssi = ctx.rrtmg_sw_taumol(inp, scon=1360.5, isolvar=2, bndscl=[0.5] * 14, indsolvar=[0.25, 1.0], solcycfrac=0.75)
    assert taug.shape == taur.shape == (NCOL, 112, NLAY) and ssi.shape == (NCOL, 112)
    expect(stub, "geosrad_rrtmg_sw_taumol", {"ncol": NCOL, "nlay": NLAY, "scon": 1360.5, "isolvar": 2, **sv, "taug": addr(taug), "taur": addr(taur),
                                             "ssi": addr(ssi), **{k: addr(d[k]) for k in ["play", "plev", "tlay"] + api._SW_GAS}})
    o = ctx.rrtmg_sw_cldprmc(inp, iceflg=2, liqflg=1)
    assert len(o) == 3 and all(x.shape == (NCOL, 112, NLAY) for x in o)
    expect(stub, "geosrad_rrtmg_sw_cldprmc", {"ncol": NCOL, "nlay": NLAY, "iceflgsw": 2, "liqflgsw": 1, "dyofyr": 200, "cloudLM": 2, "cloudMH": 3,
                                              "taucmc": addr(o[0]), "ssacmc": addr(o[1]), "asmcmc": addr(o[2]),
                                              **{k: addr(d[k]) for k in ["play", "plev", "tlay", "cld", "ciwp", "clwp", "rei", "rel", "zm", "alat"]
                                                 + api._SW_GAS}})


def test_rrtmg_dev(ctx, stub):
    """the solver entry points on device addresses: each array parameter is ptr[its name]; a name left out is NULL"""
    lw = fake(pointers("geosrad_rrtmg_lw_na_dev"), 0x100000)
    del lw["band_output"], lw["rat_gas"]
    scal = {"stream": STREAM, "ncol": NCOL, "nlay": NLAY, "psize": 4, "dudTs": 1, "iceflglw": 3, "liqflglw": 1, "dyofyr": 200, "cloudLM": 2, "cloudMH": 3}
    bo = [1, 0] * 8
    plain = {k: lw[k] for k in pointers("geosrad_rrtmg_lw_dev") if k != "band_output"}
    ctx.rrtmg_lw_dev(STREAM, NCOL, NLAY, True, lw, 3, 1, 200, 2, 3, band_output=bo)
    expect(stub, "geosrad_rrtmg_lw_dev", {**scal, **plain, "band_output": bool})
    assert stub.last("geosrad_rrtmg_lw_dev")[1]["band_output"] == bo
    part = {k: v for k, v in lw.items() if k not in ("tauaer", "olrb")}
    ctx.rrtmg_lw_dev(STREAM, NCOL, NLAY, False, part, 3, 1, 200, 2, 3)
    expect(stub, "geosrad_rrtmg_lw_dev", {**scal, **plain, "dudTs": 0, "tauaer": None, "olrb": None, "band_output": bool})
    assert stub.last("geosrad_rrtmg_lw_dev")[1]["band_output"] == [0] * 16
    rats = {k: lw[k] for k in ("uflx_rat", "dflx_rat", "duflx_dTs_rat")}
    ctx.rrtmg_lw_rats_dev(STREAM, NCOL, NLAY, True, lw, 3, 1, 200, 2, 3, ["CH4", 7], band_output=bo)
    expect(stub, "geosrad_rrtmg_lw_rats_dev", {**scal, **plain, **rats, "band_output": bool, "nrats": NRATS, "rat_gas": bool})
    assert stub.last("geosrad_rrtmg_lw_rats_dev")[1]["rat_gas"] == [3, 7]
    ctx.rrtmg_lw_na_dev(STREAM, NCOL, NLAY, True, lw, 3, 1, 200, 2, 3, rat_gas=["O3", "CO2"])
    expect(stub, "geosrad_rrtmg_lw_na_dev", {**scal, **lw, "band_output": bool, "nrats": NRATS, "rat_gas": bool})
    assert stub.last("geosrad_rrtmg_lw_na_dev")[1]["rat_gas"] == [1, 2]
    ctx.rrtmg_lw_na_dev(STREAM, NCOL, NLAY, True, lw, 3, 1, 200, 2, 3)
    expect(stub, "geosrad_rrtmg_lw_na_dev", {**scal, **lw, "band_output": bool, "nrats": 0, "rat_gas": lambda a: True})

    key = PYKEY["rrtmg_sw"]
    host = ("bndscl", "indsolvar", "solcycfrac")
    names = [p for p in pointers("geosrad_rrtmg_sw_radval_dev") if p not in host]
    sw = fake([key.get(p, p) for p in names], 0x200000)
    got = {p: sw[key.get(p, p)] for p in names}
    scal = dict(SW_SCAL, stream=STREAM)
    sv = {"bndscl": first(ctx, 0.5), "indsolvar": first(ctx, 0.25), "solcycfrac": first(ctx, 0.75)}
    args = (STREAM, NCOL, NLAY, 1360.5, 1.25, 1, sw, 3, 1, 200, 10, 2, 3)
    kw = dict(normFlx=1, do_drfband=True, bndscl=[0.5] * 14, indsolvar=[0.25, 1.0], rpart=6, solcycfrac=0.75)
    ctx.rrtmg_sw_dev(*args, **kw)
    expect(stub, "geosrad_rrtmg_sw_dev", {**scal, **sv, **{p: v for p, v in got.items() if p != "radval"}})
    ctx.rrtmg_sw_radval_dev(*args, **kw)
    expect(stub, "geosrad_rrtmg_sw_radval_dev", {**scal, **sv, **got})
    part = {k: v for k, v in sw.items() if k not in ("tauaer_sw", "drband", "radval")}
    ctx.rrtmg_sw_dev(STREAM, NCOL, NLAY, 1361.0, 1.0, 0, part, 3, 1, 200, 0, 2, 3, radval=True)
    expect(stub, "geosrad_rrtmg_sw_radval_dev", {**scal, **got, "rpart": 4, "scon": 1361.0, "adjes": 1.0, "isolvar": 0, "iaer": 0, "normFlx": 0,
                                                 "do_drfband": 0, "tauaer": None, "drband": None, "radval": None, **{k: None for k in host}})

    key = PYKEY["mcica"]
    names = [p for p in pointers("geosrad_mcica_dev") if p != "seed_order"]
    mc = fake([key.get(p, p) for p in names], 0x300000)
    ctx.generate_stochastic_clouds_dev(STREAM, NCOL, NSUB, NLAY, mc, 200, 1e-6, seed_order=(4, 3, 2, 1))
    expect(stub, "geosrad_mcica_dev", {"stream": STREAM, "ncol": NCOL, "nsubcol": NSUB, "nlay": NLAY, "doy": 200, "cwp_tiny": 1e-6, "seed_order": bool,
                                       **{p: mc[key.get(p, p)] for p in names}})
    assert stub.last("geosrad_mcica_dev")[1]["seed_order"] == [4, 3, 2, 1]


def test_chou_solvers(ctx, stub):
    rng = np.random.default_rng(4)
    m, n, ns, nb = NCOL, NLAY, 2, NBAER
    d = reals(ctx, rng, ple=(n + 1, m), ta=(n, m), wa=(n, m), oa=(n, m), tb=m, n2o=(n, m), ch4=(n, m), cfc11=(n, m), cfc12=(n, m), cfc22=(n, m),
              cwc=(4, n, m), fcld=(n, m), reff=(4, n, m), fs=(ns, m), tg=(ns, m), eg=(10, ns, m), tv=(ns, m), ev=(10, ns, m), rv=(10, ns, m))
    aer = reals(ctx, rng, taua=(nb, n, m), ssaa=(nb, n, m), asya=(nb, n, m))
    o = ctx.irrad(m, n, d["ple"], d["ta"], d["wa"], d["oa"], d["tb"], 4e-4, True, d["n2o"], d["ch4"], d["cfc11"], d["cfc12"], d["cfc22"], d["cwc"],
                  d["fcld"], 2, 3, d["reff"], ns, d["fs"], d["tg"], d["eg"], d["tv"], d["ev"], d["rv"], 1, nb, aer["taua"], aer["ssaa"], aer["asya"])
    outs = ["flxu", "flcu", "flau", "flxau", "flxd", "flcd", "flad", "flxad", "dfdts", "sfcem", "taudiag"]
    assert set(o) == set(outs) | set(aer) and o["flxu"].shape == (n + 1, m) and o["sfcem"].shape == (m,) and o["taudiag"].shape == (10, n, m)
    for k in aer:                                   # in-out: the library gets a copy, which is returned
        assert not np.shares_memory(o[k], aer[k]) and np.array_equal(o[k], aer[k])
    scal = {"m": m, "np": n, "co2": 4e-4, "trace": 1, "ict": 2, "icb": 3, "ns": ns, "na": 1, "nb": nb}
    expect(stub, "geosrad_irrad", {**scal, **{k: addr(v) for k, v in d.items()}, **{k: addr(o[k]) for k in outs + list(aer)}})
    ch = dict(d, co2=4e-4, ict=2, icb=3, ns=ns, na=0, nb=nb, taua=None, ssaa=None, asya=None)
    o = ctx.irrad_columns(ch, trace=False)
    expect(stub, "geosrad_irrad", {**scal, "trace": 0, "na": 0, **{k: addr(v) for k, v in d.items()}, **{k: addr(o[k]) for k in outs},
                                   "taua": None, "ssaa": None, "asya": None})
    ptr = fake(pointers("geosrad_irrad_dev"), 0x400000)
    ctx.irrad_dev(STREAM, m, n, ptr, 4e-4, True, 2, 3, ns, 1, nb)
    expect(stub, "geosrad_irrad_dev", {**scal, "stream": STREAM, **ptr})

    s = reals(ctx, rng, cosz=m, pl=(n + 1, m), ta=(n, m), wa=(n, m), oa=(n, m), cwc=(4, n, m), fcld=(n, m), reff=(4, n, m), hk_uv=5, hk_ir=(10, 3),
              taua=(8, n, m), ssaa=(8, n, m), asya=(8, n, m), rsuvbm=m, rsuvdf=m, rsirbm=m, rsirdf=m)
    args = (m, n, 8, s["cosz"], s["pl"], s["ta"], s["wa"], s["oa"], 4e-4, s["cwc"], s["fcld"], 2, 3, s["reff"], s["hk_uv"], s["hk_ir"], s["taua"],
            s["ssaa"], s["asya"], s["rsuvbm"], s["rsuvdf"], s["rsirbm"], s["rsirdf"])
    outs = ["flx", "flc", "fdiruv", "fdifuv", "fdirpar", "fdifpar", "fdirir", "fdifir", "flxu", "flcu", "flx_sfc_band"]
    scal = {"m": m, "np": n, "nb": 8, "co2": 4e-4, "ict": 2, "icb": 3}
    o = ctx.sorad(*args)
    assert set(o) == set(outs) and o["flx"].shape == (n + 1, m) and o["fdiruv"].shape == (m,) and o["flx_sfc_band"].shape == (8, m)
    expect(stub, "geosrad_sorad", {**scal, "do_drfband": 0, "drband": None, "dfband": None, **{k: addr(v) for k, v in s.items()},
                                   **{k: addr(o[k]) for k in outs}})
    o = ctx.sorad(*args, do_drfband=True)
    assert o["drband"].shape == o["dfband"].shape == (8, m)
    expect(stub, "geosrad_sorad", {**scal, "do_drfband": 1, **{k: addr(v) for k, v in s.items()}, **{k: addr(o[k]) for k in outs + ["drband", "dfband"]}})
    o = ctx.sorad_na(*args)
    assert set(o) == set(outs) | set(G.SONA_OUT) and o["flx_na"].shape == (n + 1, m) and o["flx_sfc_band_na"].shape == (8, m)
    want = {**scal, "do_drfband": 0, "drband": None, "dfband": None, **{k: addr(v) for k, v in s.items()}}
    expect(stub, "geosrad_sorad_na", {**want, **{k: addr(o[k]) for k in outs}}, tables={"na_out": {k: addr(o[k]) for k in G.SONA_OUT}})
    cs = dict(s, co2=4e-4, ict=2, icb=3, nb=8)
    o = ctx.sorad_na_columns(cs, na=["flc_na", "flx_sfc_band_na"])
    assert set(o) == set(outs) | {"flc_na", "flx_sfc_band_na"}
    expect(stub, "geosrad_sorad_na", {**want, **{k: addr(o[k]) for k in outs}}, tables={"na_out": {k: addr(o[k]) for k in ("flc_na", "flx_sfc_band_na")}})
    o = ctx.sorad_columns(cs)
    expect(stub, "geosrad_sorad", {**want, **{k: addr(o[k]) for k in outs}})

    ptr = fake([p for p in pointers("geosrad_sorad_dev") if p not in ("hk_uv", "hk_ir")], 0x500000)
    hk = {"hk_uv": first(ctx, s["hk_uv"][0]), "hk_ir": first(ctx, s["hk_ir"][0, 0])}
    ctx.sorad_dev(STREAM, m, n, 8, ptr, 4e-4, 2, 3, s["hk_uv"], s["hk_ir"], do_drfband=True)
    expect(stub, "geosrad_sorad_dev", {**scal, "stream": STREAM, "do_drfband": 1, **hk, **ptr})
    na = fake(G.SONA_OUT[:3], 0x600000)
    ctx.sorad_na_dev(STREAM, m, n, 8, ptr, 4e-4, 2, 3, s["hk_uv"], s["hk_ir"], na_ptr=na)
    expect(stub, "geosrad_sorad_na_dev", {**scal, "stream": STREAM, "do_drfband": 0, **hk, **ptr}, tables={"na_out": na})
    ctx.sorad_na_dev(STREAM, m, n, 8, {k: v for k, v in ptr.items() if k != "drband"}, 4e-4, 2, 3, s["hk_uv"], s["hk_ir"])
    expect(stub, "geosrad_sorad_na_dev", {**scal, "stream": STREAM, "do_drfband": 0, **hk, **ptr, "drband": None}, tables={"na_out": None})


def test_mcica_host(ctx, stub):
    rng = np.random.default_rng(5)
    d = reals(ctx, rng, zmid=(NLAY, NCOL), alat=NCOL, play=(NLAY, NCOL), cldfrac=(NLAY, NCOL), ciwp=(NLAY, NCOL), clwp=(NLAY, NCOL))
    cldy, ci, cl = ctx.generate_stochastic_clouds(NCOL, NSUB, NLAY, d["zmid"], d["alat"], 200, d["play"], d["cldfrac"], d["ciwp"], d["clwp"], 1e-6)
    assert cldy.shape == ci.shape == cl.shape == (NCOL, NSUB, NLAY) and cldy.dtype == np.int32 and ci.dtype == cl.dtype == ctx.dtype
    expect(stub, "geosrad_mcica", {"ncol": NCOL, "nsubcol": NSUB, "nlay": NLAY, "doy": 200, "cwp_tiny": 1e-6, "seed_order": bool, "cldy_stoch": addr(cldy),
                                   "ciwp_stoch": addr(ci), "clwp_stoch": addr(cl), **{k: addr(v) for k, v in d.items()}})
    assert stub.last("geosrad_mcica")[1]["seed_order"] == [1, 2, 3, 4]
    cnt = ctx.clearCounts_threeBand(NCOL, NSUB, NLAY, 2, 3, cldy)
    assert cnt.shape == (NCOL, 4) and cnt.dtype == np.int32
    expect(stub, "geosrad_clearcounts", {"ncol": NCOL, "nsubcol": NSUB, "nlay": NLAY, "cloudLM": 2, "cloudMH": 3, "cldy_stoch": addr(cldy),
                                         "clearCnts": addr(cnt)})


def test_lit_compaction_and_obio(ctx, stub, monkeypatch):
    p = fake(["zth", "lit_index", "lit_pos", "nlit_dev", "unpacked", "packed"], 0x700000)
    assert ctx.lit_index_dev(STREAM, NCOL, p["zth"], p["lit_index"], p["lit_pos"], p["nlit_dev"]) == NLIT
    expect(stub, "geosrad_lit_index_dev", {"stream": STREAM, "ncol": NCOL, "nlit_host": bool, **{k: p[k] for k in ("zth", "lit_index", "lit_pos", "nlit_dev")}})
    assert ctx.lit_index_dev(STREAM, NCOL, p["zth"], p["lit_index"], p["lit_pos"], p["nlit_dev"], want_count=False) is None
    expect(stub, "geosrad_lit_index_dev", {"stream": STREAM, "ncol": NCOL, "nlit_host": None, **{k: p[k] for k in ("zth", "lit_index", "lit_pos", "nlit_dev")}})
    ctx.lit_pack_dev(STREAM, NLIT, NCOL, NLAY, p["lit_index"], p["nlit_dev"], p["unpacked"], p["packed"])
    expect(stub, "geosrad_lit_pack_dev", {"stream": STREAM, "pdim": NLIT, "udim": NCOL, "nlev": NLAY,
                                          **{k: p[k] for k in ("lit_index", "nlit_dev", "unpacked", "packed")}})
    ctx.lit_unpack_dev(STREAM, NLIT, NCOL, NLAY, p["lit_pos"], p["packed"], p["unpacked"])
    want = {"stream": STREAM, "pdim": NLIT, "udim": NCOL, "nlev": NLAY, **{k: p[k] for k in ("lit_pos", "packed", "unpacked")}}
    expect(stub, "geosrad_lit_unpack_dev", {**want, "use_default": 0, "dflt": 0.0})
    ctx.lit_unpack_dev(STREAM, NLIT, NCOL, NLAY, p["lit_pos"], p["packed"], p["unpacked"], default=1e15)
    expect(stub, "geosrad_lit_unpack_dev", {**want, "use_default": 1, "dflt": 1e15})

    o = fake(["slr", "drbandn", "dfbandn", "drobio", "dfobio"], 0x800000)
    ctx.sw_update_obio_dev(STREAM, NCOL, G.OBIO_RRTMG, o["slr"], o["drbandn"], o["dfbandn"], o["drobio"], o["dfobio"])
    expect(stub, "geosrad_sw_update_obio_dev", {"stream": STREAM, "ncol": NCOL, "scheme": 1, "nbands": 14, "wvn1": None, "wvn2": None, "order": None, **o})
    ctx.sw_update_obio_dev(STREAM, NCOL, G.OBIO_BANDS, o["slr"], dfobio=o["dfobio"], bands=([100., 200.], [200., 300.], [2, 1]))
    expect(stub, "geosrad_sw_update_obio_dev", {"stream": STREAM, "ncol": NCOL, "scheme": 2, "nbands": 2, "wvn1": bool, "wvn2": bool, "order": bool,
                                                "slr": o["slr"], "drbandn": None, "dfbandn": None, "drobio": None, "dfobio": o["dfobio"]})
    _, mem = stub.last("geosrad_sw_update_obio_dev")
    assert mem["wvn1"] == [100., 200.] and mem["wvn2"] == [200., 300.]
    monkeypatch.setattr(_lib, "lib", lambda: stub)
    w, npairs = api.obio_weights(G.OBIO_CHOU, ctx.real_kind)
    assert w.shape == (8, 33) and w.dtype == np.float64 and npairs == 5
    expect(stub, "geosrad_obio_weights", {"scheme": 0, "real_kind": ctx.real_kind, "nbands": 8, "wvn1": None, "wvn2": None, "order": None,
                                          "weights": addr(w), "npairs": bool})
    w, _ = api.obio_weights(G.OBIO_BANDS, ctx.real_kind, bands=([100., 200.], [200., 300.], [2, 1]))
    assert w.shape == (2, 33) and stub.last("geosrad_obio_weights")[1]["wvn2"] == [200., 300.]
    stub.rc["geosrad_obio_weights"] = 1
    FIXED["geosrad_last_error"] = b"bad scheme"
    try:
        with pytest.raises(api.GeosradError, match="bad scheme") as e:
            api.obio_weights(9, ctx.real_kind)
        assert e.value.rc == 1 and stub.last("geosrad_last_error")[0]["ctx"] is None
    finally:
        del stub.rc["geosrad_obio_weights"], FIXED["geosrad_last_error"]


def tables_of(name, *skip):
    """ptr for the `in` / `out` / `rat_out` tables of an entry point (one name of each left out), and the expected tables"""
    tabs = {p: getattr(G, lst) for p, (lst, _) in TABLES[family(name)].items() if p != "na_out" and p in [q for _, q in PROTOS[name][1]]}
    ptr = {}
    for i, (p, names) in enumerate(tabs.items()):
        ptr.update(fake([k for k in names if k not in skip and k != names[1]], 0x10000 * (i + 1) + 0x900000))
    return ptr, {p: ptr for p in tabs}


def test_gridcomp_tables(ctx, stub, counters):
    for lst, cnt in {v for t in TABLES.values() for v in t.values()}:
        assert len(getattr(G, lst)) == counters[cnt], (lst, cnt)
    bo = [0, 1] * 8
    # ---- LW_Driver, RRTMG
    scal = {"stream": STREAM, "ncol": NCOL, "lm": NLAY, "nb_aer": NBAER, "consts": bool, "iceflglw": 3, "liqflglw": 1, "doy": 200, "lcldlm": 3, "lcldmh": 2,
            "band_output": bool}
    args = (STREAM, NCOL, NLAY, NBAER)
    cs = [float(i) + 0.5 for i in range(len(G.LWD_CONST))]
    ptr, tabs = tables_of("geosrad_lw_driver_rrtmg_na_dev")
    plain = {k: tabs[k] for k in ("in", "out")}
    ctx.lw_driver_rrtmg_dev(*args, ptr, cs, 3, 1, 200, 3, 2, band_output=bo)
    expect(stub, "geosrad_lw_driver_rrtmg_dev", scal, plain)
    _, mem = stub.last("geosrad_lw_driver_rrtmg_dev")
    assert mem["band_output"] == bo and mem["consts"] == cs[:2] and mem["in"][0] and mem["in"][1] is None and mem["out"][1] is None
    assert len(mem["in"]) == counters["LWD_NIN"] and len(mem["out"]) == counters["LWD_NOUT"]
    ctx.lw_driver_rrtmg_rats_dev(*args, ptr, cs, 3, 1, 200, 3, 2, ["H2O", "HCFC22"])
    expect(stub, "geosrad_lw_driver_rrtmg_rats_dev", {**scal, "nrats": NRATS, "rat_gas": bool}, tabs)
    _, mem = stub.last("geosrad_lw_driver_rrtmg_rats_dev")
    assert mem["rat_gas"] == [0, 7] and mem["band_output"] == [0] * 16
    na = fake(G.LWNA_OUT[2:], 0xA00000)
    ctx.lw_driver_rrtmg_na_dev(*args, ptr, cs, 3, 1, 200, 3, 2, na, rat_gas=["CO2", 4], band_output=bo)
    expect(stub, "geosrad_lw_driver_rrtmg_na_dev", {**scal, "nrats": NRATS, "rat_gas": bool}, {**tabs, "na_out": na})
    assert stub.last("geosrad_lw_driver_rrtmg_na_dev")[1]["rat_gas"] == [2, 4]
    ctx.lw_driver_rrtmg_na_dev(*args, ptr, cs, 3, 1, 200, 3, 2, None)
    expect(stub, "geosrad_lw_driver_rrtmg_na_dev", {**scal, "nrats": 0, "rat_gas": lambda a: True}, {**tabs, "na_out": None})
    # ---- the entry points that take only scalars and the two tables
    ptr, tabs = tables_of("geosrad_lw_update_rats_dev")
    ctx.lw_update_rats_dev(STREAM, NCOL, NLAY, NRATS, ptr)
    expect(stub, "geosrad_lw_update_rats_dev", {"stream": STREAM, "ncol": NCOL, "lm": NLAY, "nrats": NRATS}, tabs)
    ptr, tabs = tables_of("geosrad_sw_update_surface_dev")
    ctx.sw_update_surface_dev(STREAM, NCOL, NLAY, 1e15, ptr)
    expect(stub, "geosrad_sw_update_surface_dev", {"stream": STREAM, "ncol": NCOL, "lm": NLAY, "undef": 1e15}, tabs)
    ptr, tabs = tables_of("geosrad_sw_update_clouds_dev")
    ctx.sw_update_clouds_dev(STREAM, NCOL, NLAY, 2, 3, 0.1, ptr)
    expect(stub, "geosrad_sw_update_clouds_dev", {"stream": STREAM, "ncol": NCOL, "lm": NLAY, "lcldmh": 2, "lcldlm": 3, "taucrit": 0.1, "consts": bool}, tabs)
    assert stub.last("geosrad_sw_update_clouds_dev")[1]["consts"] == G.swk_consts()
    ctx.sw_update_clouds_dev(STREAM, NCOL, NLAY, 2, 3, 0.1, ptr, consts=[9.5, 1e10])
    assert stub.last("geosrad_sw_update_clouds_dev")[1]["consts"] == [9.5, 1e10]
    ptr, tabs = tables_of("geosrad_sw_update_cldhb_dev")
    ctx.sw_update_cldhb_dev(STREAM, NCOL, NLAY, 2, 3, 200, ptr)
    expect(stub, "geosrad_sw_update_cldhb_dev", {"stream": STREAM, "ncol": NCOL, "lm": NLAY, "lcldmh": 2, "lcldlm": 3, "doy": 200, "consts": None}, tabs)
    ctx.sw_update_cldhb_dev(STREAM, NCOL, NLAY, 2, 3, 200, ptr, consts=[9.5, 287.5])
    assert stub.last("geosrad_sw_update_cldhb_dev")[1]["consts"] == [9.5, 287.5]
    ptr, tabs = tables_of("geosrad_lw_driver_chou_dev")
    ctx.lw_driver_chou_dev(STREAM, NCOL, NLAY, ptr, [4e-4, 0.25, 1e15, 0.3], True, 2, 3, binary_clouds=True)
    expect(stub, "geosrad_lw_driver_chou_dev", {"stream": STREAM, "ncol": NCOL, "lm": NLAY, "consts": bool, "trace": 1, "lcldmh": 2, "lcldlm": 3,
                                                "binary_clouds": 1}, tabs)
    assert stub.last("geosrad_lw_driver_chou_dev")[1]["consts"] == [4e-4, 0.25]
    ptr, tabs = tables_of("geosrad_lw_chou_post_dev")
    ctx.lw_chou_post_dev(STREAM, NCOL, NLAY, ptr)
    expect(stub, "geosrad_lw_chou_post_dev", {"stream": STREAM, "ncol": NCOL, "lm": NLAY}, tabs)
    ptr, tabs = tables_of("geosrad_lw_update_flx_dev")
    ctx.lw_update_flx_dev(STREAM, NCOL, NLAY, False, 2, 3, 1e15, ptr)
    expect(stub, "geosrad_lw_update_flx_dev", {"stream": STREAM, "ncol": NCOL, "lm": NLAY, "rrtmg": 0, "lev_mid_high": 2, "lev_low_mid": 3, "undef": 1e15}, tabs)
    ptr, tabs = tables_of("geosrad_sw_update_export_dev")
    ctx.sw_update_export_dev(STREAM, NCOL, NLAY, 14, ptr)
    expect(stub, "geosrad_sw_update_export_dev", {"stream": STREAM, "ncol": NCOL, "lm": NLAY, "nbands": 14}, tabs)
    ptr, tabs = tables_of("geosrad_rad_tendencies_dev")
    ctx.rad_tendencies_dev(STREAM, NCOL, NLAY, 9.80665, 1004.5, ptr)
    expect(stub, "geosrad_rad_tendencies_dev", {"stream": STREAM, "ncol": NCOL, "lm": NLAY, "grav": 9.80665, "cp": 1004.5}, tabs)
    key = PYKEY["lw_update_bands"]
    ptr = fake(list(key.values()), 0xB00000)
    del ptr["TBRB_EXP"]
    ctx.lw_update_bands_dev(STREAM, NCOL, bo, 1e15, ptr)
    expect(stub, "geosrad_lw_update_bands_dev", {"stream": STREAM, "ncol": NCOL, "band_output": bool, "wavenum1": bool, "wavenum2": bool, "undef": 1e15,
                                                 **{p: ptr.get(k) for p, k in key.items()}})
    _, mem = stub.last("geosrad_lw_update_bands_dev")
    assert mem["band_output"] == bo and mem["wavenum1"] == G.LW_WAVENUM1 and mem["wavenum2"] == G.LW_WAVENUM2


def lit_expect(names, dark, keep):
    return ([float(dark.get(k, 0.0)) for k in names], sum(1 << names.index(k) for k in keep))


def test_sw_drivers(ctx, stub, counters):
    lit = fake(["lit_index", "lit_pos"], 0xC00000)
    # ---- RRTMG branch of SORADCORE: packed, _lit, _obio, _obio_lit
    ptr, tabs = tables_of("geosrad_sw_driver_rrtmg_dev")
    obio = fake(G.SWD_OBIO_OUT, 0xD00000)
    cs = [float(i) + 0.25 for i in range(len(G.SWD_CONST))]
    scal = {"stream": STREAM, "ncol": NCOL, "lm": NLAY, "nb_aer": NBAER, "consts": bool, "iceflgsw": 3, "liqflgsw": 1, "sc": 1360.5, "dist": 1.25, "isolvar": 2,
            "dyofyr": 200, "include_aerosols": 1, "lcldlm": 3, "lcldmh": 2, "normflx": 0, "bndsolvar": first(ctx, 0.5), "indsolvar": first(ctx, 0.25)}
    tail = (NLAY, NBAER, ptr, cs, 3, 1, 1360.5, 1.25, 2, 200, True, 3, 2)
    kw = dict(normflx=0, bndsolvar=[0.5] * 14, indsolvar=[0.25, 1.0])
    dark, keep = {"FSW": 1e15, "CLDTS": -1.0, "DFBAND": 2.5}, ("FSC", "COTLP", "DRBAND")
    dk, mask = lit_expect(G.SWD_OUT, dark, [k for k in keep if k in G.SWD_OUT])
    dko, masko = lit_expect(G.SWD_OBIO_OUT, dark, ["DRBAND"])
    litw = {"nlit": NLIT, **lit, "dark": bool, "keep_mask": mask}
    ctx.sw_driver_rrtmg_dev(STREAM, NCOL, *tail, **kw)
    expect(stub, "geosrad_sw_driver_rrtmg_dev", scal, tabs)
    assert stub.last("geosrad_sw_driver_rrtmg_dev")[1]["consts"] == cs[:2]
    ctx.sw_driver_rrtmg_dev(STREAM, NCOL, NLAY, NBAER, ptr, cs, 3, 1, 1360.5, 1.25, 2, 200, False, 3, 2)
    expect(stub, "geosrad_sw_driver_rrtmg_dev", {**scal, "include_aerosols": 0, "normflx": 1, "bndsolvar": None, "indsolvar": None}, tabs)
    ctx.sw_driver_rrtmg_lit_dev(STREAM, NCOL, NLIT, lit["lit_index"], lit["lit_pos"], *tail, **kw, dark={k: v for k, v in dark.items() if k in G.SWD_OUT},
                                keep=[k for k in keep if k in G.SWD_OUT])
    expect(stub, "geosrad_sw_driver_rrtmg_lit_dev", {**scal, **litw}, tabs)
    assert stub.last("geosrad_sw_driver_rrtmg_lit_dev")[1]["dark"] == dk and len(dk) == counters["SWD_NOUT"]
    ctx.sw_driver_rrtmg_lit_dev(STREAM, NCOL, NLIT, 0, None, *tail)
    expect(stub, "geosrad_sw_driver_rrtmg_lit_dev", {**scal, "nlit": NLIT, "lit_index": None, "lit_pos": None, "dark": None, "keep_mask": 0, "normflx": 1,
                                                     "bndsolvar": None, "indsolvar": None}, tabs)
    ctx.sw_driver_rrtmg_obio_dev(STREAM, NCOL, NLAY, NBAER, dict(ptr, **obio), cs, 3, 1, 1360.5, 1.25, 2, 200, True, 3, 2, **kw)
    expect(stub, "geosrad_sw_driver_rrtmg_obio_dev", {**scal, "drband": obio["DRBAND"], "dfband": obio["DFBAND"]}, tabs)
    ctx.sw_driver_rrtmg_obio_dev(STREAM, NCOL, *tail, **kw)
    expect(stub, "geosrad_sw_driver_rrtmg_obio_dev", {**scal, "drband": None, "dfband": None}, tabs)
    ctx.sw_driver_rrtmg_obio_lit_dev(STREAM, NCOL, NLIT, lit["lit_index"], lit["lit_pos"], NLAY, NBAER, dict(ptr, **obio), cs, 3, 1, 1360.5, 1.25, 2, 200,
                                     True, 3, 2, **kw, dark=dark, keep=keep)
    expect(stub, "geosrad_sw_driver_rrtmg_obio_lit_dev", {**scal, **litw, "dark_obio": bool, "keep_obio": masko, "drband": obio["DRBAND"],
                                                          "dfband": obio["DFBAND"]}, tabs)
    _, mem = stub.last("geosrad_sw_driver_rrtmg_obio_lit_dev")
    assert mem["dark"] == dk and mem["dark_obio"] == dko == [0.0, 2.5] and masko == 1
    # ---- Chou-Suarez branch: packed, _lit, _na, _na_lit
    ptr, tabs = tables_of("geosrad_sw_driver_chou_dev")
    cs = [4e-4, 47.5, 28.5, 1e15]
    hu, hi = np.full(5, 0.125), np.full((10, 3), 0.375)
    scal = {"stream": STREAM, "ncol": NCOL, "lm": NLAY, "consts": bool, "lcldmh": 2, "lcldlm": 3, "hk_uv": first(ctx, 0.125), "hk_ir": bool, "do_drfband": 1}
    tail = (NLAY, ptr, cs, 2, 3, hu, hi)
    dark, keep = {"FSWBAND": 1e15, "NIRR": -2.0}, ("FSW", "DFBAND")
    dk, mask = lit_expect(G.SWC_OUT, dark, keep)
    litw = {"nlit": NLIT, **lit, "dark": bool, "keep_mask": mask}
    na = fake(G.SWCNA_OUT[1:], 0xE00000)
    darkn, keepn = {"FSCNA": 3.5}, ("FSWBANDNA",)
    dkn, maskn = lit_expect(G.SWCNA_OUT, darkn, keepn)
    ctx.sw_driver_chou_dev(STREAM, NCOL, *tail, do_drfband=True)
    expect(stub, "geosrad_sw_driver_chou_dev", scal, tabs)
    assert stub.last("geosrad_sw_driver_chou_dev")[1]["consts"] == cs[:2]
    ctx.sw_driver_chou_lit_dev(STREAM, NCOL, NLIT, lit["lit_index"], lit["lit_pos"], *tail, do_drfband=True, dark=dark, keep=keep)
    expect(stub, "geosrad_sw_driver_chou_lit_dev", {**scal, **litw}, tabs)
    assert stub.last("geosrad_sw_driver_chou_lit_dev")[1]["dark"] == dk and len(dk) == counters["SWC_NOUT"]
    ctx.sw_driver_chou_lit_dev(STREAM, NCOL, NLIT, lit["lit_index"], lit["lit_pos"], NLAY, ptr, cs, 2, 3, None, None)
    expect(stub, "geosrad_sw_driver_chou_lit_dev", {**scal, "nlit": NLIT, **lit, "dark": None, "keep_mask": 0, "hk_uv": None, "hk_ir": None,
                                                    "do_drfband": 0}, tabs)
    ctx.sw_driver_chou_na_dev(STREAM, NCOL, *tail, do_drfband=True, na_ptr=na)
    expect(stub, "geosrad_sw_driver_chou_na_dev", scal, {**tabs, "na_out": na})
    ctx.sw_driver_chou_na_dev(STREAM, NCOL, *tail)
    expect(stub, "geosrad_sw_driver_chou_na_dev", {**scal, "do_drfband": 0}, {**tabs, "na_out": None})
    ctx.sw_driver_chou_na_lit_dev(STREAM, NCOL, NLIT, lit["lit_index"], lit["lit_pos"], *tail, do_drfband=True, dark=dark, keep=keep, na_ptr=na,
                                  dark_na=darkn, keep_na=keepn)
    expect(stub, "geosrad_sw_driver_chou_na_lit_dev", {**scal, **litw, "dark_na": bool, "keep_na": maskn}, {**tabs, "na_out": na})
    _, mem = stub.last("geosrad_sw_driver_chou_na_lit_dev")
    assert mem["dark"] == dk and mem["dark_na"] == dkn and maskn == 16 and len(dkn) == counters["SWCNA_NOUT"]
    ctx.sw_driver_chou_na_lit_dev(STREAM, NCOL, NLIT, lit["lit_index"], lit["lit_pos"], *tail)
    expect(stub, "geosrad_sw_driver_chou_na_lit_dev", {**scal, "do_drfband": 0, "nlit": NLIT, **lit, "dark": None, "keep_mask": 0, "dark_na": None,
                                                       "keep_na": 0}, {**tabs, "na_out": None})


def test_call_by_name_errors(ctx, tmp_path):
    """the binding's own checks: a parameter missing from a call by name, a name the prototype does not have, a C type the parser does not
    know"""
    with pytest.raises(TypeError, match="max_columns"):
        ctx._call("geosrad_set_chunk", {})
    with pytest.raises(TypeError, match="columns"):
        ctx._call("geosrad_set_chunk", {"max_columns": 4, "columns": 4})
    ctx._call("geosrad_set_chunk", {"max_columns": 4})
    text = open(HDR).read()
    assert set(_lib.parse_header(text)) == set(PROTOS)
    for bad, what in (("int geosrad_set_chunk(geosrad_ctx *ctx, float max_columns);", "geosrad_set_chunk"),
                      ("int geosrad_set_chunk(geosrad_ctx *ctx, int);", "geosrad_set_chunk"), ("long geosrad_destroy(geosrad_ctx *ctx);", "geosrad_destroy")):
        with pytest.raises(TypeError, match=what):
            _lib.parse_header(text + "\n" + bad + "\n")


def test_every_entry_point_the_binding_names_was_called(stub):
    """runs last in this file: the functions the stub saw are the exported names api.py refers to in code (a call `.geosrad_x(` or a name
    "geosrad_x" handed to the call by name), so a Context method that reaches the library cannot be left out above"""
    src = open(api.__file__).read()
    named = set(re.findall(r'[."](geosrad_[a-z_0-9]+)', src)) & set(_lib.EXPORTS)
    called = {c[0] for c in stub.calls}
    assert len(named) > 60 and named == called, (sorted(named - called), sorted(called - named))
