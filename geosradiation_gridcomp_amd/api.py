"""Host-side mirror of the reference's solver interface for the hot path, over the C ABI.

Names, argument order and meaning follow the reference's Fortran entry points so parity tests read like
calls into the reference:

    rrtmg_lw_ini()                          rrtmg_lw_init.F90:22
    rrtmg_lw(ncol, nlay, psize, dudTs, ...) rrtmg_lw_rad.F90:15-23
    rrtmg_sw_ini()                          SW rrtmg_sw_init.F90:23
    rrtmg_sw(rpart, ncol, nlay, scon, ...)  SW rrtmg_sw_rad.F90:68-124
    irrad(m, np, ple, ta, wa, oa, tb, ...)  GEOSirrad_GridComp/irrad.F90:27-35 (Chou-Suarez LW)
    sorad(m, np, nb, cosz, pl, ta, ...)     GEOSsolar_GridComp/sorad.F90:43-51 (Chou-Suarez SW)
    generate_stochastic_clouds(...)         cloud_subcol_gen.F90:132-137
    clearCounts_threeBand(...)              cloud_subcol_gen.F90:611-614
    set_inhomogeneity / unset_inhomogeneity cloud_condensate_inhomogeneity.F90:45,75
    initialize_cloud_subcol_gen(...)        cloud_subcol_gen.F90:109-111

Array convention: numpy C-order arrays whose reversed shape is the Fortran shape (Fortran
``play(ncol,nlay)`` <-> numpy ``(nlay, ncol)``), i.e. byte-identical to what the Fortran caller passes.
Where the reference would ``error stop`` a ``GeosradInputError`` carrying the reference's message is raised.
"""
import ctypes
import functools
import os
import numpy as np
from . import _lib
from . import gridcomp as G

NBNDLW = 16
NGPTLW = 140
NBNDSW = 14
NGPTSW = 112
_SW_GAS = ["h2ovmr", "o3vmr", "co2vmr", "ch4vmr", "o2vmr"]
_SW_COT = ["cotdtp", "cotdhp", "cotdmp", "cotdlp", "cotntp", "cotnhp", "cotnmp", "cotnlp"]
# The SOLAR_RADVAL dummy arguments of rrtmg_sw in the reference's order (SW/rrtmg_sw_rad.F90:86-119) = the GEOSRAD_RV_* slots of
# include/geosrad.h: 15 families (combined delta-scaled optical thickness; per phase l / i: un-scaled and delta-scaled optical thickness,
# single-scattering albedo, asymmetry parameter; delta-scaled forward-scattering fraction), each a denominator `d` and a numerator `n`
# for the whole column (tp) and the high / middle / low super-layer (hp, mp, lp)
RADVAL_FAMILIES = ["cds", "cotl", "cdsl", "coti", "cdsi", "ssal", "sdsl", "ssai", "sdsi", "asml", "adsl", "asmi", "adsi", "forl", "fori"]
RADVAL_NAMES = [f + dn + sl for f in RADVAL_FAMILIES for dn in "dn" for sl in ("tp", "hp", "mp", "lp")]

_IN2D = ["h2ovmr", "o3vmr", "co2vmr", "ch4vmr", "n2ovmr", "o2vmr", "cfc11vmr", "cfc12vmr", "cfc22vmr", "ccl4vmr",
         "cldf", "ciwp", "clwp", "rei", "rel"]
_LW_FLX = ["uflx", "dflx", "uflxc", "dflxc", "duflx_dTs", "duflxc_dTs"]

# header parameter -> key on the Python side, where the two differ (one map per solver; every other parameter is looked up under its own name)
_SW_PTR = {"cld": "cldf", "tauaer": "tauaer_sw", "ssaaer": "ssaaer_sw", "asmaer": "asmaer_sw", "clearCounts": "clearCounts_sw"}
_SW_INP = {"cld": "cldf"}
_CHOU_ARG = {"np": "np_"}
_MCICA_PTR = {"zmid": "zm", "cldfrac": "cldf"}
_LWB_PTR = {"tsinst": "TSINST", "ts_int": "TS_INT", "olrb_int": "OLRB", "dolrb_int": "DOLRB", "olrb_exp": "OLRB_EXP", "tbrb_exp": "TBRB_EXP"}

_SCALAR = {ctypes.c_int: int, ctypes.c_uint64: int, ctypes.c_size_t: int, ctypes.c_double: float}


class GeosradError(RuntimeError):
    pass


class GeosradInputError(GeosradError):
    """The reference would `error stop` on these inputs."""


@functools.lru_cache(maxsize=None)
def _params(name):
    """((parameter, int | float for a scalar, None for a pointer), ...) of the library function `name`, in the order of include/geosrad.h"""
    protos = _lib.all_prototypes()
    for more in (_lib.satsim_prototypes, _lib.misr_modis_prototypes, _lib.lidar_prototypes, _lib.radar_prototypes):
        if name not in protos:
            protos = more()
    return tuple((p, _SCALAR.get(t)) for t, p in protos[name][1])


def _args(name, vals):
    """The positional arguments of the library function `name` from `vals` = {parameter name in include/geosrad.h: value}: the header gives the
    order and the kind of each.  A scalar parameter takes a number or a bool; a pointer parameter a numpy array (its address), None (NULL),
    an address, bytes, or a ctypes array / byref.  TypeError for a parameter missing from `vals` and for a key that is no parameter."""
    params = _params(name)
    try:
        args = [vals[p] for p, _ in params]
    except KeyError:
        raise TypeError(f"{name}: no value for {[p for p, _ in params if p not in vals]}") from None
    if len(vals) != len(params):
        raise TypeError(f"{name}: the prototype has no parameter {[k for k in vals if k not in dict(params)]}")
    return [v.ctypes.data if isinstance(v, np.ndarray) else v if conv is None else conv(v) for v, (_, conv) in zip(args, params)]


def _band_output(band_output):
    return np.zeros(NBNDLW, dtype=np.int32) if band_output is None else np.ascontiguousarray(band_output, dtype=np.int32)


def _rats(rat_gas):
    """nrats / rat_gas of the RATS entry points from names of gridcomp.RAT_GAS (or their codes)"""
    rg = np.ascontiguousarray([G.RAT_GAS.index(g) if isinstance(g, str) else int(g) for g in rat_gas], dtype=np.int32)
    return {"nrats": len(rg), "rat_gas": rg}


def _doubles(vals, n=None):
    """a C array of n (default len(vals)) doubles: `consts` in a gridcomp.*_CONST order, band limits ...; None stays NULL"""
    return None if vals is None else (ctypes.c_double * (len(vals) if n is None else n))(*vals)


class Context:
    """One (GPU, precision) instance of the solver: replaces the reference's module-level state."""

    def __init__(self, real_kind=4, device=0, tables=True, devices=None):
        """device: HIP device index, or -1 = the library's choice for this process (GEOSRAD_DEVICE, else the launcher's node-local MPI
        rank modulo the device count: geosrad_pick_device).  devices = [ids]: a multi-device context (geosrad_create_multi) - the
        host-array entry points then split their columns into one contiguous shard per entry, processed concurrently."""
        self.L = _lib.lib()
        self.real_kind = int(real_kind)
        self.dtype = np.float32 if self.real_kind == 4 else np.float64
        self.h = ctypes.c_void_p()
        if devices is not None:
            ids = (ctypes.c_int * len(devices))(*[int(d) for d in devices])
            rc = self.L.geosrad_create_multi(ctypes.byref(self.h), ids, len(devices), self.real_kind)
        else:
            rc = self.L.geosrad_create(ctypes.byref(self.h), int(device), self.real_kind)
        if rc:
            raise GeosradError({2: "no usable HIP device (the product has no CPU fallback)"}.get(rc, f"geosrad_create rc={rc}"))
        if tables:
            self.rrtmg_lw_ini()
            self.rrtmg_sw_ini()
            self.irrad_ini()
            self.sorad_ini()

    def close(self):
        if self.h:
            self.L.geosrad_destroy(self.h)
            self.h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc):
        if rc:
            msg = self.L.geosrad_last_error(self.h).decode()
            err = (GeosradInputError if rc == 5 else GeosradError)(msg)
            err.rc = rc                     # the GEOSRAD_E* code of include/geosrad.h
            raise err

    def _kind(self):
        return "r4" if self.real_kind == 4 else "r8"

    # ---- calls by name: include/geosrad.h states each entry point's argument order and types (_lib.prototypes) -----------------
    def _call(self, name, vals):
        """`name`(this context, then vals[parameter] for every other parameter of the header's prototype: see _args) and _chk of
        its return code.  `vals` keeps the numpy arrays alive until the call has returned."""
        vals["ctx"] = self.h
        self._chk(getattr(self.L, name)(*_args(name, vals)))

    def _dev(self, name, ptr, rename={}, **vals):
        """a device-pointer call: every parameter of `name` not given in `vals` is a device array, ptr[parameter] (rename: parameter ->
        key of ptr; missing / 0 = NULL)"""
        for p, _ in _params(name):
            if p not in vals and p != "ctx":
                vals[p] = ptr.get(rename.get(p, p)) or None
        self._call(name, vals)

    def _host(self, name, a, out, rename={}, **vals):
        """a host-array call: a parameter of `name` not given in `vals` is the caller's argument a[parameter] (rename: parameter -> key of
        a) - an array as a contiguous one of the context's real kind, None as NULL - and otherwise the output array out[parameter]"""
        for p, scalar in _params(name):
            k = rename.get(p, p)
            if p in vals or p == "ctx":
                continue
            if k not in a:
                vals[p] = out.get(p)
            elif scalar or a[k] is None:
                vals[p] = a[k]
            else:
                vals[p] = np.ascontiguousarray(a[k], dtype=self.dtype)
        self._call(name, vals)

    def _zeros(self, spec, dtype=None):
        """{name: zeros(shape)} from [(name, shape)], in the context's real kind unless a dtype is given"""
        return {k: np.zeros(shape, dtype=dtype or self.dtype) for k, shape in spec}

    def _reals(self, **arrays):
        """host arrays the library reads in the context's real kind (hk_uv / hk_ir, bndsolvar / indsolvar ...); None stays NULL"""
        return {k: None if a is None else np.ascontiguousarray(a, dtype=self.dtype) for k, a in arrays.items()}

    def _solvar(self, bndscl, indsolvar, solcycfrac):
        """rrtmg_sw's optional solar-variability arguments"""
        return dict(self._reals(bndscl=bndscl, indsolvar=indsolvar), solcycfrac=None if solcycfrac is None else np.array([solcycfrac], dtype=self.dtype))

    @staticmethod
    def _ptr_array(names, ptr):
        arr = (ctypes.c_void_p * len(names))()
        for i, k in enumerate(names):
            arr[i] = ptr.get(k) or None
        return arr

    def _io(self, ptr, names_in, names_out):
        """the `in` / `out` pointer tables of a GridComp entry point from ptr = name -> device address (missing = not associated)"""
        return {"in": self._ptr_array(names_in, ptr), "out": self._ptr_array(names_out, ptr)}

    def _na_table(self, names, na_ptr):
        """the na_out table of an aerosol-free entry point; None = NULL (the plain call)"""
        return None if na_ptr is None else self._ptr_array(names, na_ptr)

    @staticmethod
    def _lit_args(names, lit_index, lit_pos, dark, keep):
        """lit_index / lit_pos: device addresses (None / 0 = NULL); dark: name -> UnPackIt's DEFAULT of that output (missing = 0.0), or None
        = NULL; keep: names of the outputs whose dark columns keep their values"""
        dk = None if dark is None else (ctypes.c_double * len(names))(*[float(dark.get(k, 0.0)) for k in names])
        mask = 0
        for k in keep:
            mask |= 1 << names.index(k)
        return ctypes.c_void_p(lit_index or None), ctypes.c_void_p(lit_pos or None), dk, ctypes.c_uint64(mask)

    def _lit(self, names, nlit, lit_index, lit_pos, dark, keep):
        """the arguments a `_lit` driver adds to its packed twin"""
        li, lp, dk, mask = self._lit_args(names, lit_index, lit_pos, dark, keep)
        return {"nlit": nlit, "lit_index": li, "lit_pos": lp, "dark": dk, "keep_mask": mask.value}

    # ---- initialisation ------------------------------------------------------------------------------
    def _load(self, name, tables, path):
        path = path or os.path.join(_lib.DATA, f"{tables}_{self._kind()}.grtb")
        self._call(name, {"path": os.fsencode(path)})

    def rrtmg_lw_ini(self, path=None):
        self._load("geosrad_load_tables_lw", "rrtmg_lw", path)

    def rrtmg_sw_ini(self, path=None):
        self._load("geosrad_load_tables_sw", "rrtmg_sw", path)

    def irrad_ini(self, path=None):
        """uploads irrad_constants / rad_constants (the reference keeps them as module data: no init routine there)"""
        self._load("geosrad_load_tables_chou_lw", "chou_lw", path)

    def sorad_ini(self, path=None):
        self._load("geosrad_load_tables_chou_sw", "chou_sw", path)

    def set_inhomogeneity(self, ih, path=None):
        if ih and path is None:
            path = os.path.join(_lib.DATA, f"xcw_{'beta' if ih == 1 else 'gamma'}_{self._kind()}.grtb")
        self._call("geosrad_load_inhomogeneity", {"ih": ih, "path": os.fsencode(path) if path else None})

    def unset_inhomogeneity(self):
        self.set_inhomogeneity(0)

    def initialize_cloud_subcol_gen(self, adl=None, rdl=None):
        self._call("geosrad_set_corr_lengths", {"adl": _doubles(adl, 4), "rdl": _doubles(rdl, 4)})

    def set_chunk(self, n):
        self._call("geosrad_set_chunk", {"max_columns": n})

    def workspace_bytes(self):
        return int(self.L.geosrad_workspace_bytes(self.h))

    def set_overcast(self, irrad=False, sorad=False):
        """The Chou-Suarez schemes as the reference builds them with -DOVERCAST (geosrad_set_overcast): every layer clear or fully cloudy,
        random overlap, ict / icb not read.  One switch per scheme; both off (the default) is maximum-random overlap."""
        self._call("geosrad_set_overcast", {"flags": (1 if irrad else 0) | (2 if sorad else 0)})

    @property
    def overcast(self):
        """dict(irrad=bool, sorad=bool): the current geosrad_set_overcast mode."""
        f = int(self.L.geosrad_get_overcast(self.h))
        return {"irrad": bool(f & 1), "sorad": bool(f & 2)}

    # ---- RRTMG_LW, host arrays -------------------------------------------------------------------------
    def rrtmg_lw(self, ncol, nlay, psize, dudTs, play, plev, tlay, tlev, tsfc, emis,
                 h2ovmr, o3vmr, co2vmr, ch4vmr, n2ovmr, o2vmr, cfc11vmr, cfc12vmr, cfc22vmr, ccl4vmr,
                 cldf, ciwp, clwp, rei, rel, iceflglw, liqflglw, tauaer, zm, alat, dyofyr, cloudLM, cloudMH,
                 band_output=None, out=None):
        """Returns dict(uflx,dflx,uflxc,dflxc,duflx_dTs,duflxc_dTs (nlay+1,ncol); clearCounts (4,ncol);
        olrb,dolrb_dTs (ncol,16))."""
        return self._rrtmg_lw_host("geosrad_rrtmg_lw", locals(), _LW_FLX)

    def rrtmg_lw_na(self, ncol, nlay, psize, dudTs, play, plev, tlay, tlev, tsfc, emis,
                    h2ovmr, o3vmr, co2vmr, ch4vmr, n2ovmr, o2vmr, cfc11vmr, cfc12vmr, cfc22vmr, ccl4vmr,
                    cldf, ciwp, clwp, rei, rel, iceflglw, liqflglw, tauaer, zm, alat, dyofyr, cloudLM, cloudMH,
                    band_output=None, out=None):
        """rrtmg_lw + the aerosol-free fluxes of the same call (geosrad_rrtmg_lw_na): the dict additionally holds
        uflx_na, dflx_na, uflxc_na, dflxc_na, duflx_dTs_na, duflxc_dTs_na (nlay+1,ncol)."""
        return self._rrtmg_lw_host("geosrad_rrtmg_lw_na", locals(), [k + s for k in _LW_FLX for s in ("", "_na")])

    def _rrtmg_lw_host(self, name, a, flx):
        """rrtmg_lw / rrtmg_lw_na: `a` = their arguments by name, `flx` = the (nlay+1,ncol) outputs of the entry point `name`"""
        ncol, nlay, out = a["ncol"], a["nlay"], a["out"]
        assert np.shape(a["play"]) == (nlay, ncol) and np.shape(a["plev"]) == (nlay + 1, ncol)
        if out is None:       # (a caller that keeps its output arrays, like a Fortran caller does, passes the dict of an earlier call)
            out = self._zeros([(k, (nlay + 1, ncol)) for k in flx])
            out["clearCounts"] = np.zeros((4, ncol), dtype=np.int32)
            out.update(self._zeros([("olrb", (ncol, NBNDLW)), ("dolrb_dTs", (ncol, NBNDLW))]))
        self._host(name, a, out, band_output=_band_output(a["band_output"]))
        return out

    def rrtmg_lw_na_columns(self, inp, psize=4, dudTs=True, iceflg=3, liqflg=1, band_output=None, out=None):
        """Convenience: `inp` as produced by synth.make_columns."""
        nlay, ncol = inp["play"].shape
        return self.rrtmg_lw_na(ncol, nlay, psize, dudTs, inp["play"], inp["plev"], inp["tlay"], inp["tlev"], inp["tsfc"],
                                inp["emis"], *[inp[k] for k in _IN2D], iceflg, liqflg, inp.get("tauaer"), inp["zm"],
                                inp["alat"], inp["dyofyr"], inp["cloudLM"], inp["cloudMH"], band_output=band_output, out=out)

    def rrtmg_lw_columns(self, inp, psize=4, dudTs=True, iceflg=3, liqflg=1, band_output=None, out=None):
        """Convenience: `inp` as produced by synth.make_columns."""
        nlay, ncol = inp["play"].shape
        return self.rrtmg_lw(ncol, nlay, psize, dudTs, inp["play"], inp["plev"], inp["tlay"], inp["tlev"], inp["tsfc"],
                             inp["emis"], *[inp[k] for k in _IN2D], iceflg, liqflg, inp.get("tauaer"), inp["zm"],
                             inp["alat"], inp["dyofyr"], inp["cloudLM"], inp["cloudMH"], band_output=band_output, out=out)

    def rrtmg_lw_taumol(self, inp):
        """(taug, pfracs) numpy (ncol,140,nlay) == Fortran (nlay,140,ncol), as left by the reference's taumol."""
        nlay, ncol = inp["play"].shape
        out = self._zeros([(k, (ncol, NGPTLW, nlay)) for k in ("taug", "pfracs")])
        self._host("geosrad_rrtmg_lw_taumol", inp, out, ncol=ncol, nlay=nlay)
        return out["taug"], out["pfracs"]

    # ---- RRTMG_SW, host arrays -------------------------------------------------------------------------
    def rrtmg_sw(self, rpart, ncol, nlay, scon, adjes, coszen, isolvar, play, plev, tlay, h2ovmr, o3vmr, co2vmr, ch4vmr, o2vmr,
                 iceflgsw, liqflgsw, cld, ciwp, clwp, rei, rel, dyofyr, zm, alat, iaer, tauaer, ssaaer, asmaer,
                 asdir, asdif, aldir, aldif, cloudLM, cloudMH, normFlx, do_drfband=False, bndscl=None, indsolvar=None, out=None,
                 solcycfrac=None, radval=False):
        """rrtmg_sw (SW/rrtmg_sw_rad.F90:68).  Returns dict(swuflx,swdflx,swuflxc,swdflxc (nlay+1,ncol); nirr..uvrf,
        cotdtp..cotnlp (ncol); fswband[,drband,dfband] (14,ncol); clearCounts (4,ncol)).  radval=True: the reference's SOLAR_RADVAL
        build (geosrad_rrtmg_sw_radval): also `radval` (120,ncol) and a view of each row under its name in RADVAL_NAMES."""
        a = locals()
        assert np.shape(play) == (nlay, ncol) and np.shape(plev) == (nlay + 1, ncol)
        if out is None:
            out = self._zeros([(k, (nlay + 1, ncol)) for k in ("swuflx", "swdflx", "swuflxc", "swdflxc")]
                              + [(k, ncol) for k in ["nirr", "nirf", "parr", "parf", "uvrr", "uvrf"] + _SW_COT]
                              + [(k, (NBNDSW, ncol)) for k in ["fswband"] + (["drband", "dfband"] if do_drfband else [])])
            out["clearCounts"] = np.zeros((4, ncol), dtype=np.int32)
        extra = self._solvar(bndscl, indsolvar, solcycfrac)
        if radval:
            extra["radval"] = out.setdefault("radval", np.zeros((len(RADVAL_NAMES), ncol), dtype=self.dtype))
        self._host("geosrad_rrtmg_sw_radval" if radval else "geosrad_rrtmg_sw", a, out, **extra)
        if radval:
            for k, name in enumerate(RADVAL_NAMES):
                out[name] = out["radval"][k]
        return out

    def rrtmg_sw_radval(self, *args, **kw):
        """rrtmg_sw as the reference builds it with -DSOLAR_RADVAL (SW/rrtmg_sw_rad.F90:85-120): the arguments of rrtmg_sw; the result
        also holds the 120 cloud-optics diagnostics cdsdtp .. forinlp (ncol each, keys RADVAL_NAMES)."""
        return self.rrtmg_sw(*args, radval=True, **kw)

    def rrtmg_sw_columns(self, inp, scon=1361.0, adjes=1.0, isolvar=0, iceflg=3, liqflg=1, iaer=0, normFlx=0, do_drfband=False,
                         bndscl=None, indsolvar=None, rpart=4, out=None, solcycfrac=None, radval=False):
        """Convenience: `inp` as produced by synth.make_columns.  radval=True: see rrtmg_sw_radval."""
        nlay, ncol = inp["play"].shape
        aer = [inp.get(k) if iaer == 10 else None for k in ("tauaer_sw", "ssaaer_sw", "asmaer_sw")]
        return self.rrtmg_sw(rpart, ncol, nlay, scon, adjes, inp["coszen"], isolvar, inp["play"], inp["plev"], inp["tlay"],
                             *[inp[k] for k in _SW_GAS], iceflg, liqflg, inp["cldf"], inp["ciwp"], inp["clwp"], inp["rei"], inp["rel"],
                             inp["dyofyr"], inp["zm"], inp["alat"], iaer, *aer, inp["asdir"], inp["asdif"], inp["aldir"], inp["aldif"],
                             inp["cloudLM"], inp["cloudMH"], normFlx, do_drfband=do_drfband, bndscl=bndscl, indsolvar=indsolvar, out=out,
                             solcycfrac=solcycfrac, radval=radval)

    def rrtmg_sw_taumol(self, inp, scon=1361.0, isolvar=0, bndscl=None, indsolvar=None, solcycfrac=None):
        """(taug, taur) numpy (ncol,112,nlay) and ssi (ncol,112) as left by the reference's taumol_sw."""
        nlay, ncol = inp["play"].shape
        out = self._zeros([("taug", (ncol, NGPTSW, nlay)), ("taur", (ncol, NGPTSW, nlay)), ("ssi", (ncol, NGPTSW))])
        self._host("geosrad_rrtmg_sw_taumol", inp, out, ncol=ncol, nlay=nlay, scon=scon, isolvar=isolvar,
                   **self._solvar(bndscl, indsolvar, solcycfrac))
        return out["taug"], out["taur"], out["ssi"]

    def rrtmg_sw_cldprmc(self, inp, iceflg=3, liqflg=1):
        """(taucmc, ssacmc, asmcmc) numpy (ncol,112,nlay) == Fortran (nlay,112,ncol): the cloud optics of the solver's own McICA
        sub-columns as the reference's cldprmc_sw leaves them."""
        nlay, ncol = inp["play"].shape
        out = self._zeros([(k, (ncol, NGPTSW, nlay)) for k in ("taucmc", "ssacmc", "asmcmc")])
        self._host("geosrad_rrtmg_sw_cldprmc", inp, out, _SW_INP, ncol=ncol, nlay=nlay, iceflgsw=iceflg, liqflgsw=liqflg)
        return list(out.values())

    def rrtmg_sw_dev(self, stream, ncol, nlay, scon, adjes, isolvar, ptr, iceflg, liqflg, dyofyr, iaer, cloudLM, cloudMH, normFlx=0,
                     do_drfband=False, bndscl=None, indsolvar=None, rpart=4, solcycfrac=None, radval=False):
        """`ptr`: dict name -> device address (int) for every argument array of rrtmg_sw (inputs and outputs).  radval=True
        (rrtmg_sw_radval_dev): ptr["radval"] is the (120,ncol) device array of the SOLAR_RADVAL diagnostics."""
        self._dev("geosrad_rrtmg_sw_radval_dev" if radval else "geosrad_rrtmg_sw_dev", ptr, _SW_PTR, stream=stream, rpart=rpart, ncol=ncol,
                  nlay=nlay, scon=scon, adjes=adjes, isolvar=isolvar, iceflgsw=iceflg, liqflgsw=liqflg, dyofyr=dyofyr, iaer=iaer,
                  cloudLM=cloudLM, cloudMH=cloudMH, normFlx=normFlx, do_drfband=do_drfband, **self._solvar(bndscl, indsolvar, solcycfrac))

    def rrtmg_sw_radval_dev(self, *args, **kw):
        """rrtmg_sw_dev plus ptr["radval"]: the SOLAR_RADVAL diagnostics, (120,ncol) on the device, rows in RADVAL_NAMES order."""
        return self.rrtmg_sw_dev(*args, radval=True, **kw)

    # ---- Chou-Suarez LW, host arrays ---------------------------------------------------------------------
    def irrad(self, m, np_, ple, ta, wa, oa, tb, co2, trace, n2o, ch4, cfc11, cfc12, cfc22, cwc, fcld, ict, icb, reff,
              ns, fs, tg, eg, tv, ev, rv, na, nb, taua, ssaa, asya):
        """irrad (irrad.F90:27).  Returns dict(flxu, flcu, flau, flxau, flxd, flcd, flad, flxad, dfdts (np+1, m); sfcem (m);
        taudiag (10, np, m); taua, ssaa, asya = the in-out aerosol arrays after the call)."""
        a = locals()
        assert np.shape(ple) == (np_ + 1, m) and np.shape(ta) == (np_, m)
        aer = {k: None if a[k] is None else np.array(a[k], dtype=self.dtype, order="C", copy=True) for k in ("taua", "ssaa", "asya")}
        out = self._zeros([(k, (np_ + 1, m)) for k in ("flxu", "flcu", "flau", "flxau", "flxd", "flcd", "flad", "flxad", "dfdts")]
                          + [("sfcem", m), ("taudiag", (10, np_, m))])
        self._host("geosrad_irrad", a, out, _CHOU_ARG, **aer)
        out.update(aer)
        return out

    def irrad_columns(self, ch, trace=True):
        """Convenience: `ch` as produced by synth.chou_lw_inputs."""
        n1, m = ch["ple"].shape
        return self.irrad(m, n1 - 1, ch["ple"], ch["ta"], ch["wa"], ch["oa"], ch["tb"], ch["co2"], trace, ch["n2o"], ch["ch4"], ch["cfc11"],
                          ch["cfc12"], ch["cfc22"], ch["cwc"], ch["fcld"], ch["ict"], ch["icb"], ch["reff"], ch["ns"], ch["fs"], ch["tg"],
                          ch["eg"], ch["tv"], ch["ev"], ch["rv"], ch["na"], ch["nb"], ch["taua"], ch["ssaa"], ch["asya"])

    def irrad_dev(self, stream, m, np_, ptr, co2, trace, ict, icb, ns, na, nb):
        """`ptr`: dict name -> device address for every array argument of irrad (inputs, in-out aerosols, outputs)."""
        self._dev("geosrad_irrad_dev", ptr, stream=stream, m=m, np=np_, co2=co2, trace=trace, ict=ict, icb=icb, ns=ns, na=na, nb=nb)

    # ---- gettau (include/geosrad_gettau.h): the cloud optics of GEOS_RadiationShared/gettau.F90 over a batch of columns ---------
    def _gettau_host(self, name, a, shapes, want):
        """the host-array call `name`: `a` = the caller's arguments by parameter name, `shapes` = [(output, shape)] of which `want` are
        allocated, passed and returned (the others go as NULL: neither computed nor written)"""
        unknown = set(want) - {k for k, _ in shapes}
        if unknown:
            raise TypeError(f"{name}: no output {sorted(unknown)}")
        out = self._zeros([(k, s) for k, s in shapes if k in want])
        self._host(name, a, out)
        return out

    def getvistau(self, ncol, nlevs, cosz, dp, fcld, reff, hydromets, ict, icb, grav=G.MAPL["GRAV"], want=("taubeam", "taudiff", "asycl")):
        """getvistau (gettau.F90:33) for ncol columns: cosz (ncol); dp [Pa], fcld (nlevs, ncol); reff [microns], hydromets [kg/kg]
        (4, nlevs, ncol); ict = 0: in-cloud optical thicknesses, else scaled for the overlap of the super-layers split at ict / icb.
        Returns dict(taubeam, taudiff (4, nlevs, ncol); asycl (nlevs, ncol)) of the names in `want`."""
        a = locals()
        return self._gettau_host("geosrad_getvistau", a, [("taubeam", (4, nlevs, ncol)), ("taudiff", (4, nlevs, ncol)), ("asycl", (nlevs, ncol))], want)

    def getnirtau(self, ib, ncol, nlevs, cosz, dp, fcld, reff, hydromets, ict, icb, grav=G.MAPL["GRAV"],
                  want=("taubeam", "taudiff", "asycl", "ssacl")):
        """getnirtau (gettau.F90:102) for NIR band ib = 1..3: as getvistau, plus ssacl (nlevs, ncol)."""
        a = locals()
        return self._gettau_host("geosrad_getnirtau", a, [("taubeam", (4, nlevs, ncol)), ("taudiff", (4, nlevs, ncol)), ("asycl", (nlevs, ncol)),
                                                        ("ssacl", (nlevs, ncol))], want)

    def getirtau(self, ib, ncol, nlevs, dp, fcld, reff, hydromets, grav=G.MAPL["GRAV"], want=("taudiag", "tcldlyr", "enn")):
        """getirtau (gettau.F90:173) for IR band ib = 1..10.  Returns dict(taudiag (4, nlevs, ncol); tcldlyr, enn (nlevs + 1, ncol), level
        0 = 1 / 0) of the names in `want`."""
        a = locals()
        return self._gettau_host("geosrad_getirtau", a, [("taudiag", (4, nlevs, ncol)), ("tcldlyr", (nlevs + 1, ncol)), ("enn", (nlevs + 1, ncol))], want)

    def getvistau_dev(self, stream, ncol, nlevs, ptr, ict, icb, grav=G.MAPL["GRAV"]):
        """`ptr`: name -> device address of cosz, dp, fcld, reff, hydromets and of the wanted outputs taubeam, taudiff, asycl (missing = NULL)."""
        self._dev("geosrad_getvistau_dev", ptr, stream=stream, ncol=ncol, nlevs=nlevs, ict=ict, icb=icb, grav=grav)

    def getnirtau_dev(self, stream, ib, ncol, nlevs, ptr, ict, icb, grav=G.MAPL["GRAV"]):
        """`ptr` as for getvistau_dev, plus ssacl."""
        self._dev("geosrad_getnirtau_dev", ptr, stream=stream, ib=ib, ncol=ncol, nlevs=nlevs, ict=ict, icb=icb, grav=grav)

    def getirtau_dev(self, stream, ib, ncol, nlevs, ptr, grav=G.MAPL["GRAV"]):
        """`ptr`: name -> device address of dp, fcld, reff, hydromets and of the wanted outputs taudiag, tcldlyr, enn (missing = NULL)."""
        self._dev("geosrad_getirtau_dev", ptr, stream=stream, ib=ib, ncol=ncol, nlevs=nlevs, grav=grav)

    def lw_cloud_diag_dev(self, stream, ncol, lm, ptr, taucrit=0.30, grav=G.MAPL["GRAV"], undef=G.MAPL["UNDEF"]):
        """TAUIR / CLDTMP / CLDPRS of LW_Driver for any LW scheme (GEOS_IrradGridComp.F90:1898-1912, :3626-3650): `ptr` = name -> device
        address of the GEOS fields PLE, T, FCLD, QI QL QR QS, RI RL RR RS (model ordering) and of the wanted exports TAUIR (lm, ncol), CLDTMP,
        CLDPRS (ncol); taucrit = the TAUCRIT: resource of the Irrad GridComp."""
        self._dev("geosrad_lw_cloud_diag_dev", ptr, {p: p.upper() for p, _ in _params("geosrad_lw_cloud_diag_dev")}, stream=stream, ncol=ncol, lm=lm,
                  grav=grav, undef=undef, taucrit=taucrit)

    # ---- the satellite simulator's ISCCP path (include/geosrad_satsim.h): SCOPS, ICARUS, the COSP wrapper ------------------------
    ICARUS_OUT = ("fq_isccp", "totalcldarea", "meanptop", "meantaucld", "meanalbedocld", "meantb", "meantbclr", "boxtau", "boxptop")

    def scops(self, npoints, nlev, ncol, seed, cc, conv, overlap):
        """scops (scops.f) for npoints points: seed int32 (npoints), one CONG stream each; cc, conv (nlev, npoints), TOA first.  Returns
        (frac_out (nlev, ncol, npoints) in the real kind: 0 clear, 1 stratiform, 2 convective; the seeds as the routine leaves them)."""
        seed = np.array(seed, dtype=np.int32, order="C", copy=True)
        a = dict(npoints=npoints, nlev=nlev, ncol=ncol, cc=cc, conv=conv, overlap=overlap)
        out = self._zeros([("frac_out", (nlev, ncol, npoints))])
        self._host("geosrad_scops", a, out, seed=seed)
        return out["frac_out"], seed

    def scops_dev(self, stream, npoints, nlev, ncol, ptr, overlap):
        """`ptr`: name -> device address of seed (int32, in/out), cc, conv and frac_out_u8 (one byte per cell)."""
        self._dev("geosrad_scops_dev", ptr, stream=stream, npoints=npoints, nlev=nlev, ncol=ncol, overlap=overlap)

    def icarus(self, npoints, sunlit, nlev, ncol, pfull, phalf, qv, cc, conv, dtau_s, dtau_c, top_height, top_height_direction, overlap,
               frac_out, skt, emsfc_lw, at, dem_s, dem_c, want=ICARUS_OUT):
        """icarus (icarus.f) in its own argument order, minus debug / debugcol: arrays (nlev, npoints) TOA first, phalf (nlev + 1, npoints),
        frac_out (nlev, ncol, npoints) in the real kind, sunlit int32 (npoints).  Returns dict(fq_isccp (7 pressure, 7 tau, npoints);
        totalcldarea ... meantbclr (npoints); boxtau, boxptop (ncol, npoints)) of the names in `want`; -1.E+30 = the reference's missing value."""
        a = {k: v for k, v in locals().items() if k not in ("self", "want", "sunlit")}
        unknown = set(want) - set(self.ICARUS_OUT)
        if unknown:
            raise TypeError(f"geosrad_icarus: no output {sorted(unknown)}")
        shapes = {"fq_isccp": (7, 7, npoints), "boxtau": (ncol, npoints), "boxptop": (ncol, npoints)}
        out = self._zeros([(k, shapes.get(k, (npoints,))) for k in self.ICARUS_OUT if k in want])
        self._host("geosrad_icarus", a, out, sunlit=np.ascontiguousarray(sunlit, dtype=np.int32))
        return out

    def icarus_dev(self, stream, npoints, nlev, ncol, ptr, top_height, top_height_direction, overlap, emsfc_lw):
        """`ptr`: name -> device address of sunlit (int32), pfull ... dem_c, frac_out_u8 and of the wanted outputs (missing = NULL)."""
        self._dev("geosrad_icarus_dev", ptr, stream=stream, npoints=npoints, nlev=nlev, ncol=ncol, top_height=top_height,
                  top_height_direction=top_height_direction, overlap=overlap, emsfc_lw=emsfc_lw)

    def cosp_seeds_dev(self, stream, npoints, ptr):
        """cosp.F90:167-174: `ptr` = device addresses of psfc (npoints) and seed (int32, npoints)."""
        self._dev("geosrad_cosp_seeds_dev", ptr, stream=stream, npoints=npoints)

    def isccp_dev(self, stream, npoints, lm, ncol, ptr, overlap=3, top_height=1, top_height_direction=2, emsfc_lw=0.999):
        """The COSP ISCCP path on GEOS fields in model order (defaults: GEOS_SatsimGridComp.F90:3360-3362, :3462): `ptr` = name -> device
        address of T, QV, FCLD, CCA, PLE, PLO, DTAU_S, EMISS, DTAU_C, DEM_C, TS (CCA, DTAU_C, DEM_C may be missing = zero), sunlit and seed
        (int32) and of the wanted outputs fq_isccp ... boxptop, SGFCLD (lm, npoints)."""
        up = ("T", "QV", "FCLD", "CCA", "PLE", "PLO", "DTAU_S", "EMISS", "DTAU_C", "DEM_C", "TS", "SGFCLD")
        self._dev("geosrad_isccp_dev", ptr, {k.lower(): k for k in up}, stream=stream, npoints=npoints, lm=lm, ncol=ncol, overlap=overlap,
                  top_height=top_height, top_height_direction=top_height_direction, emsfc_lw=emsfc_lw)

    # ---- the MISR simulator (include/geosrad_misr_modis.h) --------------------------------------------------------------------
    MISR_OUT = ("fq_MISR_TAU_v_CTH", "dist_model_layertops", "MISR_mean_ztop", "MISR_cldarea")

    def misr(self, npoints, nlev, ncol, sunlit, zfull, at, dtau_s, dtau_c, frac_out, missing_value, want=MISR_OUT):
        """MISR_simulator (MISR_simulator.f) in its own argument order: arrays (nlev, npoints) TOA first, frac_out (nlev, ncol, npoints) in
        the real kind, sunlit int32 (npoints).  Returns dict(fq_MISR_TAU_v_CTH (16 heights, 7 tau, npoints); dist_model_layertops (16,
        npoints); MISR_mean_ztop, MISR_cldarea (npoints)) of the names in `want`.  The pattern matcher works on the call's first point only
        and a dark point's MISR_mean_ztop is 0 unless it is the call's last: the reference's behaviour (include/geosrad_misr_modis.h)."""
        a = {k: v for k, v in locals().items() if k not in ("self", "want", "sunlit")}
        unknown = set(want) - set(self.MISR_OUT)
        if unknown:
            raise TypeError(f"geosrad_misr: no output {sorted(unknown)}")
        shapes = {"fq_MISR_TAU_v_CTH": (16, 7, npoints), "dist_model_layertops": (16, npoints)}
        out = self._zeros([(k, shapes.get(k, (npoints,))) for k in self.MISR_OUT if k in want])
        self._host("geosrad_misr", a, out, sunlit=np.ascontiguousarray(sunlit, dtype=np.int32))
        return out

    def misr_dev(self, stream, npoints, nlev, ncol, ptr, missing_value):
        """`ptr`: name -> device address of sunlit (int32), zfull, at, dtau_s, dtau_c, frac_out_u8 (one byte per cell) and of the wanted
        outputs fq_MISR_TAU_v_CTH, dist_model_layertops, MISR_mean_ztop, MISR_cldarea (missing = NULL)."""
        self._dev("geosrad_misr_dev", ptr, stream=stream, npoints=npoints, nlev=nlev, ncol=ncol, missing_value=missing_value)

    # ---- the MODIS simulator and the whole COSP path (include/geosrad_misr_modis.h) ------------------------------------------
    MODIS_OUT = ("modis_mean", "modis_hist", "phase", "ctp", "tau", "size")
    MODIS_MEAN = ("cf_total", "cf_water", "cf_ice", "cf_high", "cf_mid", "cf_low", "tau_total", "tau_water", "tau_ice", "logtau_total", "logtau_water",
                  "logtau_ice", "size_water", "size_ice", "ctp_total", "lwp", "iwp")          # the GEOSRAD_MODIS_* indices of modis_mean

    def modis(self, npoints, nlev, ncol, sunlit, t, p, ph, dtau_s, dtau_c, frac_out, mr_lsliq, mr_lsice, mr_cvliq, mr_cvice, reff_lsliq,
              reff_lsice, reff_cvliq, reff_cvice, isccp_boxtau, isccp_boxptop, want=("modis_mean", "modis_hist")):
        """COSP_Modis_Simulator on gridbox-level fields (nlev, npoints) TOA first, ph (nlev + 1, npoints), frac_out (nlev, ncol, npoints) in the
        real kind, isccp_boxtau / isccp_boxptop (ncol, npoints); dtau_c and the convective arrays may be None (zero), isccp_boxtau too (not
        read).  Returns dict(modis_mean (17, npoints) in MODIS_MEAN's order; modis_hist (7 pressure, 7 tau, npoints); phase int32, ctp, tau,
        size (ncol, npoints)) of the names in `want`; -1.0E30 where the reference leaves R_UNDEF."""
        a = {k: v for k, v in locals().items() if k not in ("self", "want", "sunlit")}
        unknown = set(want) - set(self.MODIS_OUT)
        if unknown:
            raise TypeError(f"geosrad_modis: no output {sorted(unknown)}")
        shapes = {"modis_mean": (17, npoints), "modis_hist": (7, 7, npoints)}
        out = {k: np.zeros(shapes.get(k, (ncol, npoints)), dtype=np.int32 if k == "phase" else self.dtype) for k in self.MODIS_OUT if k in want}
        self._host("geosrad_modis", a, out, sunlit=np.ascontiguousarray(sunlit, dtype=np.int32))
        return out

    def modis_dev(self, stream, npoints, nlev, ncol, ptr):
        """`ptr`: name -> device address of sunlit (int32), t, p, ph, dtau_s, dtau_c, frac_out_u8, mr_lsliq ... reff_cvice, isccp_boxtau,
        isccp_boxptop and of the wanted outputs modis_mean, modis_hist, phase (int32), ctp, tau, size (missing = NULL)."""
        self._dev("geosrad_modis_dev", ptr, stream=stream, npoints=npoints, nlev=nlev, ncol=ncol)

    def cosp_dev(self, stream, npoints, lm, ncol, ptr, overlap=3, top_height=1, top_height_direction=2, emsfc_lw=0.999):
        """call COSP with the ISCCP, MISR and MODIS simulators on, on GEOS fields in model order: `ptr` as for isccp_dev, plus ZLE (lm + 1,
        npoints), QLTOT, QITOT, RDFL, RDFI (lm, npoints) and the wanted outputs fq_MISR_TAU_v_CTH, dist_model_layertops, MISR_mean_ztop,
        MISR_cldarea, modis_mean, modis_hist.  An output group that is missing altogether skips that simulator."""
        up = ("T", "QV", "FCLD", "CCA", "PLE", "PLO", "DTAU_S", "EMISS", "DTAU_C", "DEM_C", "TS", "SGFCLD", "ZLE", "QLTOT", "QITOT", "RDFL", "RDFI")
        self._dev("geosrad_cosp_dev", ptr, {k.lower(): k for k in up}, stream=stream, npoints=npoints, lm=lm, ncol=ncol, overlap=overlap,
                  top_height=top_height, top_height_direction=top_height_direction, emsfc_lw=emsfc_lw)

    # ---- the lidar simulator and the COSP path with it (include/geosrad_lidar.h) ------------------------------------------------
    LIDAR_OUT = ("lidarcld", "cldlayer", "cfad_sr", "parasolrefl", "pmol", "beta_tot", "tau_tot", "refl")
    LIDAR_CAT = ("low", "mid", "high", "total")          # the GEOSRAD_LIDAR_* indices of cldlayer

    def lidar(self, npoints, nlev, ncol, ice_type, p, t, presf, pplay, frac_out, mr_lsliq, mr_lsice, mr_cvliq, mr_cvice, reff_lsliq,
              reff_lsice, reff_cvliq, reff_cvice, land, want=("lidarcld", "cldlayer", "cfad_sr", "parasolrefl", "pmol")):
        """COSP_LIDAR and diag_lidar on gridbox-level fields (nlev, npoints) TOA first, presf (nlev + 1, npoints), frac_out (nlev, ncol, npoints)
        in the real kind, land (npoints); the convective arrays may be None (zero).  Returns dict(lidarcld, pmol (nlev, npoints); cldlayer (4,
        npoints) in LIDAR_CAT's order; cfad_sr (nlev, 15, npoints); parasolrefl (5, npoints); beta_tot, tau_tot (nlev, ncol, npoints); refl (5,
        ncol, npoints)) of the names in `want`; -1.0E30 where the reference leaves R_UNDEF."""
        a = {k: v for k, v in locals().items() if k not in ("self", "want")}
        unknown = set(want) - set(self.LIDAR_OUT)
        if unknown:
            raise TypeError(f"geosrad_lidar: no output {sorted(unknown)}")
        shapes = {"lidarcld": (nlev, npoints), "cldlayer": (4, npoints), "cfad_sr": (nlev, 15, npoints), "parasolrefl": (5, npoints),
                  "pmol": (nlev, npoints), "beta_tot": (nlev, ncol, npoints), "tau_tot": (nlev, ncol, npoints), "refl": (5, ncol, npoints)}
        out = self._zeros([(k, shapes[k]) for k in self.LIDAR_OUT if k in want])
        self._host("geosrad_lidar", a, out)
        return out

    def lidar_dev(self, stream, npoints, nlev, ncol, ice_type, ptr):
        """`ptr`: name -> device address of p, t, presf, pplay, frac_out_u8 (one byte per cell), mr_lsliq ... reff_cvice, land and of the
        wanted outputs lidarcld, cldlayer, cfad_sr, parasolrefl, pmol, beta_tot, tau_tot, refl (missing = NULL)."""
        self._dev("geosrad_lidar_dev", ptr, stream=stream, npoints=npoints, nlev=nlev, ncol=ncol, ice_type=ice_type)

    def cosp_lidar_dev(self, stream, npoints, lm, ncol, ptr, overlap=3, top_height=1, top_height_direction=2, emsfc_lw=0.999, ice_type=0):
        """call COSP with the ISCCP, MISR, MODIS and lidar simulators on, on GEOS fields in model order: `ptr` as for cosp_dev, plus FROCEAN
        (npoints) and the wanted lidar outputs clcalipso, lidarpmol (lm, npoints), cldlayer (4, npoints), cfad_sr (lm, 15, npoints), parasolrefl
        (5, npoints).  An output group that is missing altogether skips that simulator.  ice_type: GEOS_SatsimGridComp.F90:3535 sets 0."""
        up = ("T", "QV", "FCLD", "CCA", "PLE", "PLO", "DTAU_S", "EMISS", "DTAU_C", "DEM_C", "TS", "SGFCLD", "ZLE", "QLTOT", "QITOT", "RDFL", "RDFI",
              "FROCEAN")
        self._dev("geosrad_cosp_lidar_dev", ptr, {k.lower(): k for k in up}, stream=stream, npoints=npoints, lm=lm, ncol=ncol, overlap=overlap,
                  top_height=top_height, top_height_direction=top_height_direction, emsfc_lw=emsfc_lw, ice_type=ice_type)

    # ---- the radar simulator's front end (include/geosrad_radar.h) ------------------------------------------------------------
    HYDRO = ("lsliq", "lsice", "lsrain", "lssnow", "cvliq", "cvice", "cvrain", "cvsnow", "lsgrpl")          # the GEOSRAD_HYDRO_* indices
    SGHYDRO_OUT = ("prec_frac", "frac_ls", "frac_cv", "prec_ls", "prec_cv", "mr_sub", "mr_hydro_sg")

    def prec_scops(self, npoints, nlev, ncol, ls_p_rate, cv_p_rate, frac_out):
        """prec_scops (llnl/prec_scops.f) in its own argument order: the rates (nlev, npoints) TOA first, frac_out (nlev, ncol, npoints) in
        the real kind.  Returns prec_frac (nlev, ncol, npoints) in the real kind: 0 clear, 1 large-scale, 2 convective, 3 both."""
        a = dict(npoints=npoints, nlev=nlev, ncol=ncol, ls_p_rate=ls_p_rate, cv_p_rate=cv_p_rate, frac_out=frac_out)
        out = self._zeros([("prec_frac", (nlev, ncol, npoints))])
        self._host("geosrad_prec_scops", a, out)
        return out["prec_frac"]

    def prec_scops_dev(self, stream, npoints, nlev, ncol, ptr):
        """`ptr`: name -> device address of ls_p_rate, cv_p_rate, frac_out_u8 and prec_frac_u8 (one byte per cell)."""
        self._dev("geosrad_prec_scops_dev", ptr, stream=stream, npoints=npoints, nlev=nlev, ncol=ncol)

    def cosp_sghydro(self, npoints, nlev, ncol, frac_out, mr_lsliq, mr_lsice, mr_lsrain, mr_lssnow, mr_cvliq=None, mr_cvice=None, mr_cvrain=None,
                     mr_cvsnow=None, mr_lsgrpl=None, want=("prec_frac", "frac_ls", "frac_cv", "prec_ls", "prec_cv", "mr_sub")):
        """The sub-grid hydrometeor contents of cosp.F90:399-519 from the SCOPS mask frac_out (nlev, ncol, npoints) in the real kind and the
        gridbox mixing ratios (nlev, npoints) TOA first; the convective ones and the graupel may be None (zero).  Returns dict(prec_frac (nlev,
        ncol, npoints); frac_ls, frac_cv, prec_ls, prec_cv (nlev, npoints); mr_sub (9, nlev, npoints) in HYDRO's order; mr_hydro_sg (9, nlev,
        ncol, npoints)) of the names in `want`."""
        a = {k: v for k, v in locals().items() if k not in ("self", "want")}
        unknown = set(want) - set(self.SGHYDRO_OUT)
        if unknown:
            raise TypeError(f"geosrad_cosp_sghydro: no output {sorted(unknown)}")
        shapes = {"prec_frac": (nlev, ncol, npoints), "mr_sub": (9, nlev, npoints), "mr_hydro_sg": (9, nlev, ncol, npoints)}
        out = self._zeros([(k, shapes.get(k, (nlev, npoints))) for k in self.SGHYDRO_OUT if k in want])
        self._host("geosrad_cosp_sghydro", a, out)
        return out

    def cosp_sghydro_dev(self, stream, npoints, nlev, ncol, ptr):
        """`ptr`: name -> device address of frac_out_u8 (one byte per cell), mr_lsliq ... mr_lsgrpl and of the wanted outputs prec_frac_u8,
        frac_ls, frac_cv, prec_ls, prec_cv, mr_sub, mr_hydro_sg (missing = NULL)."""
        self._dev("geosrad_cosp_sghydro_dev", ptr, stream=stream, npoints=npoints, nlev=nlev, ncol=ncol)

    def radar_gases(self, npoints, nlev, p, t, rh, zlev, freq, surface_radar=0, want=("g_vol", "g_to_vol")):
        """gases (quickbeam/gases.f90) for every volume and path_integral to every gate (radar_simulator.f90:470-484): p (Pa), t (K), rh (%),
        zlev (m) (nlev, npoints) TOA first, freq in GHz.  Returns dict(g_vol dB/km, g_to_vol dB (nlev, npoints)), float64 in either kind."""
        a = {k: v for k, v in locals().items() if k not in ("self", "want")}
        unknown = set(want) - {"g_vol", "g_to_vol"}
        if unknown:
            raise TypeError(f"geosrad_radar_gases: no output {sorted(unknown)}")
        out = self._zeros([(k, (nlev, npoints)) for k in ("g_vol", "g_to_vol") if k in want], dtype=np.float64)
        self._host("geosrad_radar_gases", a, out)
        return out

    def radar_gases_dev(self, stream, npoints, nlev, ptr, freq, surface_radar=0):
        """`ptr`: name -> device address of p, t, rh, zlev and of the wanted outputs g_vol, g_to_vol (doubles; missing = NULL)."""
        self._dev("geosrad_radar_gases_dev", ptr, stream=stream, npoints=npoints, nlev=nlev, freq=freq, surface_radar=surface_radar)

    # ---- Chou-Suarez SW, host arrays ---------------------------------------------------------------------
    def sorad(self, m, np_, nb, cosz, pl, ta, wa, oa, co2, cwc, fcld, ict, icb, reff, hk_uv, hk_ir, taua, ssaa, asya,
              rsuvbm, rsuvdf, rsirbm, rsirdf, do_drfband=False):
        """sorad (sorad.F90:43).  Returns dict(flx, flc, flxu, flcu (np+1, m); fdiruv ... fdifir (m); flx_sfc_band[, drband, dfband] (8, m))."""
        return self._sorad_host(m, np_, nb, cosz, pl, ta, wa, oa, co2, cwc, fcld, ict, icb, reff, hk_uv, hk_ir, taua, ssaa, asya,
                                rsuvbm, rsuvdf, rsirbm, rsirdf, do_drfband, None)

    def sorad_na(self, m, np_, nb, cosz, pl, ta, wa, oa, co2, cwc, fcld, ict, icb, reff, hk_uv, hk_ir, taua, ssaa, asya,
                 rsuvbm, rsuvdf, rsirbm, rsirdf, do_drfband=False, na=None):
        """sorad + the aerosol-free fluxes of the same columns from the same call (geosrad_sorad_na): the dict additionally holds
        flx_na, flc_na, flxu_na, flcu_na (np+1, m) and flx_sfc_band_na (8, m).  `na`: the gridcomp.SONA_OUT names to take (default all;
        the others are passed as NULL and not returned)."""
        return self._sorad_host(m, np_, nb, cosz, pl, ta, wa, oa, co2, cwc, fcld, ict, icb, reff, hk_uv, hk_ir, taua, ssaa, asya,
                                rsuvbm, rsuvdf, rsirbm, rsirdf, do_drfband, G.SONA_OUT if na is None else list(na))

    def sorad_na_columns(self, cs, do_drfband=False, na=None):
        """Convenience: `cs` as produced by synth.chou_sw_inputs."""
        n1, m = cs["pl"].shape
        return self.sorad_na(m, n1 - 1, cs["nb"], cs["cosz"], cs["pl"], cs["ta"], cs["wa"], cs["oa"], cs["co2"], cs["cwc"], cs["fcld"],
                             cs["ict"], cs["icb"], cs["reff"], cs["hk_uv"], cs["hk_ir"], cs["taua"], cs["ssaa"], cs["asya"], cs["rsuvbm"],
                             cs["rsuvdf"], cs["rsirbm"], cs["rsirdf"], do_drfband=do_drfband, na=na)

    def _sorad_host(self, m, np_, nb, cosz, pl, ta, wa, oa, co2, cwc, fcld, ict, icb, reff, hk_uv, hk_ir, taua, ssaa, asya,
                    rsuvbm, rsuvdf, rsirbm, rsirdf, do_drfband, na):
        """geosrad_sorad (na None) or geosrad_sorad_na with the gridcomp.SONA_OUT names in `na`"""
        a = locals()
        assert np.shape(pl) == (np_ + 1, m) and np.shape(hk_uv) == (5,) and np.shape(hk_ir) == (10, 3)
        out = self._zeros([(k, (np_ + 1, m)) for k in ("flx", "flc", "flxu", "flcu")]
                          + [(k, m) for k in ("fdiruv", "fdifuv", "fdirpar", "fdifpar", "fdirir", "fdifir")]
                          + [(k, (8, m)) for k in ["flx_sfc_band"] + (["drband", "dfband"] if do_drfband else [])])
        if na is None:
            self._host("geosrad_sorad", a, out, _CHOU_ARG)
        else:
            out.update(self._zeros([(k, (8, m) if k == "flx_sfc_band_na" else (np_ + 1, m)) for k in na]))
            self._host("geosrad_sorad_na", a, out, _CHOU_ARG, na_out=self._ptr_array(G.SONA_OUT, {k: out[k].ctypes.data for k in na}))
        return out

    def sorad_columns(self, cs, do_drfband=False):
        """Convenience: `cs` as produced by synth.chou_sw_inputs."""
        n1, m = cs["pl"].shape
        return self.sorad(m, n1 - 1, cs["nb"], cs["cosz"], cs["pl"], cs["ta"], cs["wa"], cs["oa"], cs["co2"], cs["cwc"], cs["fcld"], cs["ict"],
                          cs["icb"], cs["reff"], cs["hk_uv"], cs["hk_ir"], cs["taua"], cs["ssaa"], cs["asya"], cs["rsuvbm"], cs["rsuvdf"],
                          cs["rsirbm"], cs["rsirdf"], do_drfband=do_drfband)

    def sorad_dev(self, stream, m, np_, nb, ptr, co2, ict, icb, hk_uv, hk_ir, do_drfband=False):
        """`ptr`: dict name -> device address for every array argument of sorad; hk_uv / hk_ir are host arrays."""
        self._dev("geosrad_sorad_dev", ptr, stream=stream, m=m, np=np_, nb=nb, co2=co2, ict=ict, icb=icb, do_drfband=do_drfband,
                  **self._reals(hk_uv=hk_uv, hk_ir=hk_ir))

    def sorad_na_dev(self, stream, m, np_, nb, ptr, co2, ict, icb, hk_uv, hk_ir, do_drfband=False, na_ptr=None):
        """sorad_dev + the aerosol-free fluxes of the same call (geosrad_sorad_na_dev): `na_ptr` = name -> device address for
        gridcomp.SONA_OUT ((np+1, m), flx_sfc_band_na (8, m); missing = NULL, left untouched; None = na_out NULL, the plain call)."""
        self._dev("geosrad_sorad_na_dev", ptr, stream=stream, m=m, np=np_, nb=nb, co2=co2, ict=ict, icb=icb, do_drfband=do_drfband,
                  na_out=self._na_table(G.SONA_OUT, na_ptr), **self._reals(hk_uv=hk_uv, hk_ir=hk_ir))

    # ---- RRTMG_LW, device pointers (bench / drivers that keep data in HBM) -------------------------------------
    def _rrtmg_lw_dev(self, name, stream, ncol, nlay, dudTs, ptr, iceflg, liqflg, dyofyr, cloudLM, cloudMH, band_output, **extra):
        """the three RRTMG_LW device entry points: the plain one, and what `extra` and further names of `ptr` add to it"""
        self._dev(name, ptr, stream=stream, ncol=ncol, nlay=nlay, psize=4, dudTs=dudTs, iceflglw=iceflg, liqflglw=liqflg, dyofyr=dyofyr,
                  cloudLM=cloudLM, cloudMH=cloudMH, band_output=_band_output(band_output), **extra)

    def rrtmg_lw_dev(self, stream, ncol, nlay, dudTs, ptr, iceflg, liqflg, dyofyr, cloudLM, cloudMH, band_output=None):
        """`ptr`: dict name -> device address (int) for every argument array of rrtmg_lw (inputs and outputs)."""
        self._rrtmg_lw_dev("geosrad_rrtmg_lw_dev", stream, ncol, nlay, dudTs, ptr, iceflg, liqflg, dyofyr, cloudLM, cloudMH, band_output)

    def rrtmg_lw_rats_dev(self, stream, ncol, nlay, dudTs, ptr, iceflg, liqflg, dyofyr, cloudLM, cloudMH, rat_gas, band_output=None):
        """rrtmg_lw_dev + the RATS loop of LW_Driver (GEOS_IrradGridComp.F90:3405-3468) from the same call: `rat_gas` = names from
        gridcomp.RAT_GAS; ptr["uflx_rat"], ["dflx_rat"], ["duflx_dTs_rat"] = device arrays [len(rat_gas)][nlay+1][ncol]."""
        self._rrtmg_lw_dev("geosrad_rrtmg_lw_rats_dev", stream, ncol, nlay, dudTs, ptr, iceflg, liqflg, dyofyr, cloudLM, cloudMH, band_output,
                           **_rats(rat_gas))

    def rrtmg_lw_na_dev(self, stream, ncol, nlay, dudTs, ptr, iceflg, liqflg, dyofyr, cloudLM, cloudMH, rat_gas=(), band_output=None):
        """rrtmg_lw_rats_dev (`rat_gas` may be empty) + the aerosol-free fluxes of the same call (geosrad_rrtmg_lw_na_dev):
        ptr["uflx_na"], ["dflx_na"], ["uflxc_na"], ["dflxc_na"], and with dudTs ["duflx_dTs_na"], ["duflxc_dTs_na"] = device arrays
        [nlay+1][ncol].  A call of the band-partials path throughout, like one with RATS diagnostics."""
        self._rrtmg_lw_dev("geosrad_rrtmg_lw_na_dev", stream, ncol, nlay, dudTs, ptr, iceflg, liqflg, dyofyr, cloudLM, cloudMH, band_output,
                           **_rats(rat_gas))

    # ---- GridComp data path either side of the solvers (device pointers, GEOS layout) ---------------------------------------
    def _lw_driver_rrtmg(self, name, stream, ncol, lm, nb_aer, ptr, consts, iceflg, liqflg, doy, lcldlm, lcldmh, band_output, **extra):
        """the three RRTMG LW_Driver entry points: the plain one, and what `extra` adds to it"""
        self._call(name, dict(extra, stream=stream, ncol=ncol, lm=lm, nb_aer=nb_aer, consts=_doubles(consts, len(G.LWD_CONST)),
                              iceflglw=iceflg, liqflglw=liqflg, doy=doy, lcldlm=lcldlm, lcldmh=lcldmh, band_output=_band_output(band_output),
                              **self._io(ptr, G.LWD_IN, G.LWD_OUT)))

    def lw_driver_rrtmg_dev(self, stream, ncol, lm, nb_aer, ptr, consts, iceflg, liqflg, doy, lcldlm, lcldmh, band_output=None):
        """RRTMG branch of LW_Driver (GEOS_IrradGridComp.F90:3188-3615).  `ptr`: name -> device address for gridcomp.LWD_IN and
        gridcomp.LWD_OUT (missing / 0 = not associated); `consts` in gridcomp.LWD_CONST order; lcldlm / lcldmh in MODEL ordering."""
        self._lw_driver_rrtmg("geosrad_lw_driver_rrtmg_dev", stream, ncol, lm, nb_aer, ptr, consts, iceflg, liqflg, doy, lcldlm, lcldmh,
                              band_output)

    def lw_driver_rrtmg_rats_dev(self, stream, ncol, lm, nb_aer, ptr, consts, iceflg, liqflg, doy, lcldlm, lcldmh, rat_gas,
                                 band_output=None):
        """lw_driver_rrtmg_dev with the RATS loop (IRR:3389-3469, :3522-3530, :3614): `rat_gas` = names from gridcomp.RAT_GAS,
        `ptr` additionally holds gridcomp.LWD_RAT_OUT ((nrats, LM+1, ncol), SFCEM_RAT (nrats, ncol); missing = not associated)."""
        self._lw_driver_rrtmg("geosrad_lw_driver_rrtmg_rats_dev", stream, ncol, lm, nb_aer, ptr, consts, iceflg, liqflg, doy, lcldlm, lcldmh,
                              band_output, rat_out=self._ptr_array(G.LWD_RAT_OUT, ptr), **_rats(rat_gas))

    def lw_driver_rrtmg_na_dev(self, stream, ncol, lm, nb_aer, ptr, consts, iceflg, liqflg, doy, lcldlm, lcldmh, na_ptr, rat_gas=(),
                               band_output=None):
        """lw_driver_rrtmg_rats_dev (`rat_gas` may be empty) with the aerosol-free INTERNALs of the same solver call
        (geosrad_lw_driver_rrtmg_na_dev): `na_ptr` = name -> device address for gridcomp.LWNA_OUT ((LM+1, ncol); missing = not
        associated; None = none of them).  Its DFDTSNA / DFDTSCNA are the real derivatives; ptr["DFDTSNA"] stays the reference's copy.
        lw_update_flx_dev(rrtmg=False) reads the INTERNALs so filled."""
        self._lw_driver_rrtmg("geosrad_lw_driver_rrtmg_na_dev", stream, ncol, lm, nb_aer, ptr, consts, iceflg, liqflg, doy, lcldlm, lcldmh,
                              band_output, rat_out=self._ptr_array(G.LWD_RAT_OUT, ptr), na_out=self._na_table(G.LWNA_OUT, na_ptr),
                              **_rats(rat_gas))

    def lw_update_rats_dev(self, stream, ncol, lm, nrats, ptr):
        """RATS exports of Update_Flx (GEOS_IrradGridComp.F90:4036-4120).  `ptr`: name -> device address for gridcomp.LWR_IN and
        gridcomp.LWR_OUT (missing = export not associated)."""
        self._call("geosrad_lw_update_rats_dev", dict(stream=stream, ncol=ncol, lm=lm, nrats=nrats, **self._io(ptr, G.LWR_IN, G.LWR_OUT)))

    def lw_update_bands_dev(self, stream, ncol, band_output, undef, ptr):
        """Band OLR / brightness-temperature exports of Update_Flx (GEOS_IrradGridComp.F90:3993-4021).  `ptr`: TSINST, TS_INT, OLRB,
        DOLRB (internals, (ncol,16) C order) and the exports OLRB_EXP, TBRB_EXP ((16,ncol) C order; missing = not associated)."""
        self._dev("geosrad_lw_update_bands_dev", ptr, _LWB_PTR, stream=stream, ncol=ncol, band_output=np.ascontiguousarray(band_output, dtype=np.int32),
                  wavenum1=_doubles(G.LW_WAVENUM1), wavenum2=_doubles(G.LW_WAVENUM2), undef=undef)

    def sw_update_surface_dev(self, stream, ncol, lm, undef, ptr):
        """2-D block of UPDATE_EXPORT (GEOS_SolarGridComp.F90:7403-7533): `ptr` name -> device address for gridcomp.SWS_IN / SWS_OUT
        (the albedo exports are named ALBVF_X ...; missing = not associated)."""
        self._call("geosrad_sw_update_surface_dev", dict(stream=stream, ncol=ncol, lm=lm, undef=undef, **self._io(ptr, G.SWS_IN, G.SWS_OUT)))

    def sw_update_clouds_dev(self, stream, ncol, lm, lcldmh, lcldlm, taucrit, ptr, consts=None):
        """cloud diagnostics of UPDATE_EXPORT (GEOS_SolarGridComp.F90:7006-7058, :7223-7392): `ptr` name -> device address for
        gridcomp.SWK_IN / SWK_OUT (missing = not associated); lcldmh / lcldlm in model ordering; taucrit = the TAUCRIT: resource (0.10);
        consts in gridcomp.SWK_CONST order (default gridcomp.swk_consts())."""
        self._call("geosrad_sw_update_clouds_dev", dict(
            stream=stream, ncol=ncol, lm=lm, lcldmh=lcldmh, lcldlm=lcldlm, taucrit=taucrit,
            consts=_doubles(G.swk_consts() if consts is None else consts, len(G.SWK_CONST)), **self._io(ptr, G.SWK_IN, G.SWK_OUT)))

    def sw_update_cldhb_dev(self, stream, ncol, lm, lcldmh, lcldlm, doy, ptr, consts=None):
        """heartbeat McICA cloud fractions CLD??SWHB of UPDATE_EXPORT (GEOS_SolarGridComp.F90:7060-7223, SOLAR_RADVAL): `ptr` name -> device
        address for gridcomp.SWHB_IN / SWHB_OUT (a missing export = not associated); lcldmh / lcldlm in model ordering; doy = day of the
        year (the correlation lengths); consts in gridcomp.SWHB_CONST order (default: the library's MAPL_GRAV and MAPL_RGAS).  The context's
        set_inhomogeneity / initialize_cloud_subcol_gen settings apply, as for generate_stochastic_clouds_dev."""
        self._call("geosrad_sw_update_cldhb_dev", dict(stream=stream, ncol=ncol, lm=lm, lcldmh=lcldmh, lcldlm=lcldlm, doy=doy,
                                                       consts=_doubles(consts, len(G.SWHB_CONST)), **self._io(ptr, G.SWHB_IN, G.SWHB_OUT)))

    def _sw_driver_rrtmg(self, name, stream, ncol, lm, nb_aer, ptr, consts, iceflg, liqflg, sc, dist, isolvar, dyofyr, include_aerosols,
                         lcldlm, lcldmh, normflx, bndsolvar, indsolvar, **extra):
        """the four RRTMG SORADCORE entry points: the packed one, and what `extra` adds to it (_lit: the un-packed tile; _obio: DRBAND / DFBAND)"""
        self._call(name, dict(extra, stream=stream, ncol=ncol, lm=lm, nb_aer=nb_aer, consts=_doubles(consts, len(G.SWD_CONST)),
                              iceflgsw=iceflg, liqflgsw=liqflg, sc=sc, dist=dist, isolvar=isolvar, dyofyr=dyofyr,
                              include_aerosols=include_aerosols, lcldlm=lcldlm, lcldmh=lcldmh, normflx=normflx,
                              **self._reals(bndsolvar=bndsolvar, indsolvar=indsolvar), **self._io(ptr, G.SWD_IN, G.SWD_OUT)))

    @staticmethod
    def _obio_out(ptr):
        return {"drband": ptr.get("DRBAND") or None, "dfband": ptr.get("DFBAND") or None}      # gridcomp.SWD_OBIO_OUT

    def sw_driver_rrtmg_dev(self, stream, ncol, lm, nb_aer, ptr, consts, iceflg, liqflg, sc, dist, isolvar, dyofyr, include_aerosols,
                            lcldlm, lcldmh, normflx=1, bndsolvar=None, indsolvar=None):
        """RRTMG branch of SORADCORE on the packed daytime columns (GEOS_SolarGridComp.F90:6113-6450)."""
        self._sw_driver_rrtmg("geosrad_sw_driver_rrtmg_dev", stream, ncol, lm, nb_aer, ptr, consts, iceflg, liqflg, sc, dist, isolvar, dyofyr,
                              include_aerosols, lcldlm, lcldmh, normflx, bndsolvar, indsolvar)

    def _sw_driver_chou(self, name, stream, ncol, lm, ptr, consts, lcldmh, lcldlm, hk_uv, hk_ir, do_drfband, **extra):
        """the four Chou-Suarez SORADCORE entry points: the packed one, and what `extra` adds to it (_lit: the un-packed tile; _na: FS*NA)"""
        self._call(name, dict(extra, stream=stream, ncol=ncol, lm=lm, consts=_doubles(consts, len(G.SWC_CONST)), lcldmh=lcldmh, lcldlm=lcldlm,
                              do_drfband=do_drfband, **self._reals(hk_uv=hk_uv, hk_ir=hk_ir), **self._io(ptr, G.SWC_IN, G.SWC_OUT)))

    def sw_driver_chou_dev(self, stream, ncol, lm, ptr, consts, lcldmh, lcldlm, hk_uv, hk_ir, do_drfband=False):
        """Chou-Suarez branch of SORADCORE on the packed daytime columns (GEOS_SolarGridComp.F90:4484-4572, SHRTWAVE :6597-6672):
        `ptr` holds device pointers of gridcomp.SWC_IN (TAUA / SSAA / ASYA may be missing: no aerosols) and gridcomp.SWC_OUT;
        consts in the order of gridcomp.SWC_CONST; hk_uv (5) and hk_ir (memory order of the Fortran (3,10), as for sorad_dev) host arrays
        (HK_UV_TEMP, HK_IR_TEMP)."""
        self._sw_driver_chou("geosrad_sw_driver_chou_dev", stream, ncol, lm, ptr, consts, lcldmh, lcldlm, hk_uv, hk_ir, do_drfband)

    def sw_driver_chou_na_dev(self, stream, ncol, lm, ptr, consts, lcldmh, lcldlm, hk_uv, hk_ir, do_drfband=False, na_ptr=None):
        """sw_driver_chou_dev + the aerosol-free internals FSWNA, FSCNA, FSWUNA, FSCUNA, FSWBANDNA from the same prep and the same solver
        call (geosrad_sw_driver_chou_na_dev; the reference runs SORADCORE a second time, GEOS_SolarGridComp.F90:3249-3259): `na_ptr` =
        name -> device address for gridcomp.SWCNA_OUT (missing = not associated; None = none of them)."""
        self._sw_driver_chou("geosrad_sw_driver_chou_na_dev", stream, ncol, lm, ptr, consts, lcldmh, lcldlm, hk_uv, hk_ir, do_drfband,
                             na_out=self._na_table(G.SWCNA_OUT, na_ptr))

    def sw_driver_chou_na_lit_dev(self, stream, ncol, nlit, lit_index, lit_pos, lm, ptr, consts, lcldmh, lcldlm, hk_uv, hk_ir,
                                  do_drfband=False, dark=None, keep=(), na_ptr=None, dark_na=None, keep_na=()):
        """sw_driver_chou_na_dev on the un-packed tile: see sw_driver_chou_lit_dev; dark_na / keep_na by gridcomp.SWCNA_OUT name."""
        na = self._lit(G.SWCNA_OUT, nlit, lit_index, lit_pos, dark_na, keep_na)
        self._sw_driver_chou("geosrad_sw_driver_chou_na_lit_dev", stream, ncol, lm, ptr, consts, lcldmh, lcldlm, hk_uv, hk_ir, do_drfband,
                             **self._lit(G.SWC_OUT, nlit, lit_index, lit_pos, dark, keep), dark_na=na["dark"], keep_na=na["keep_mask"],
                             na_out=self._na_table(G.SWCNA_OUT, na_ptr))

    def sw_driver_rrtmg_lit_dev(self, stream, ncol, nlit, lit_index, lit_pos, lm, nb_aer, ptr, consts, iceflg, liqflg, sc, dist, isolvar,
                                dyofyr, include_aerosols, lcldlm, lcldmh, normflx=1, bndsolvar=None, indsolvar=None, dark=None, keep=()):
        """sw_driver_rrtmg_dev on the un-packed tile of ncol columns, nlit of them lit (GEOS_SolarGridComp.F90:3686, PackIt :3839-3894,
        UnPackIt :6520-6580): `ptr` holds tile-wide fields, lit_index / lit_pos / nlit are what lit_index_dev gave; dark / keep as in
        _lit_args, by gridcomp.SWD_OUT name.  TAUA / SSAA / ASYA are only read."""
        self._sw_driver_rrtmg("geosrad_sw_driver_rrtmg_lit_dev", stream, ncol, lm, nb_aer, ptr, consts, iceflg, liqflg, sc, dist, isolvar, dyofyr,
                              include_aerosols, lcldlm, lcldmh, normflx, bndsolvar, indsolvar,
                              **self._lit(G.SWD_OUT, nlit, lit_index, lit_pos, dark, keep))

    def sw_driver_chou_lit_dev(self, stream, ncol, nlit, lit_index, lit_pos, lm, ptr, consts, lcldmh, lcldlm, hk_uv, hk_ir, do_drfband=False,
                               dark=None, keep=()):
        """sw_driver_chou_dev on the un-packed tile of ncol columns, nlit of them lit: see sw_driver_rrtmg_lit_dev; dark / keep by
        gridcomp.SWC_OUT name."""
        self._sw_driver_chou("geosrad_sw_driver_chou_lit_dev", stream, ncol, lm, ptr, consts, lcldmh, lcldlm, hk_uv, hk_ir, do_drfband,
                             **self._lit(G.SWC_OUT, nlit, lit_index, lit_pos, dark, keep))

    def lw_driver_chou_dev(self, stream, ncol, lm, ptr, consts, trace, lcldmh, lcldlm, binary_clouds=False):
        """Chou-Suarez branch of LW_Driver in one call (GEOS_IrradGridComp.F90:1781-1785, :1876-1912, :2093-2108, :3604-3663): `ptr` holds
        device pointers of gridcomp.LWK_IN (TAUA / SSAA / ASYA may be missing: no aerosols; when given they are rescaled in place like
        irrad does) and gridcomp.LWK_OUT (LWK_OUT_REQUIRED must be there, the rest missing = not associated); consts in the order of
        gridcomp.LWK_CONST (gridcomp.lwk_consts()); lcldmh / lcldlm: irrad's ict / icb; binary_clouds: RADLW_BINARY_CLOUDS."""
        self._call("geosrad_lw_driver_chou_dev", dict(stream=stream, ncol=ncol, lm=lm, consts=_doubles(consts, len(G.LWK_CONST)), trace=trace,
                                                      lcldmh=lcldmh, lcldlm=lcldlm, binary_clouds=binary_clouds, **self._io(ptr, G.LWK_IN, G.LWK_OUT)))

    def lw_chou_post_dev(self, stream, ncol, lm, ptr):
        """after irrad in the Chou-Suarez branch of LW_Driver (GEOS_IrradGridComp.F90:2101-2108, :3601-3616): gridcomp.LWC_IN / LWC_OUT"""
        self._call("geosrad_lw_chou_post_dev", dict(stream=stream, ncol=ncol, lm=lm, **self._io(ptr, G.LWC_IN, G.LWC_OUT)))

    def lw_update_flx_dev(self, stream, ncol, lm, rrtmg, lev_mid_high, lev_low_mid, undef, ptr):
        """Update_Flx (GEOS_IrradGridComp.F90:3796-3999): `ptr` holds gridcomp.LWU_IN internals and the requested gridcomp.LWU_OUT."""
        self._call("geosrad_lw_update_flx_dev", dict(stream=stream, ncol=ncol, lm=lm, rrtmg=rrtmg, lev_mid_high=lev_mid_high,
                                                     lev_low_mid=lev_low_mid, undef=undef, **self._io(ptr, G.LWU_IN, G.LWU_OUT)))

    def sw_update_export_dev(self, stream, ncol, lm, nbands, ptr):
        """flux part of UPDATE_EXPORT (GEOS_SolarGridComp.F90:7540-7579)."""
        self._call("geosrad_sw_update_export_dev", dict(stream=stream, ncol=ncol, lm=lm, nbands=nbands, **self._io(ptr, G.SWU_IN, G.SWU_OUT)))

    def sw_update_obio_dev(self, stream, ncol, scheme, slr, drbandn=None, dfbandn=None, drobio=None, dfobio=None, bands=None):
        """SOLAR TO OBIO conversion of UPDATE_EXPORT (GEOS_SolarGridComp.F90:7584-7737): device addresses of SLR (ncol), DRBANDN / DFBANDN
        (ncol,nbands) and the exports DROBIO / DFOBIO (ncol,33); None / 0 = not associated.  scheme: gridcomp.OBIO_CHOU | OBIO_RRTMG, or
        OBIO_BANDS with bands = (wvn1, wvn2, order) as for obio_weights."""
        self._call("geosrad_sw_update_obio_dev", dict(_obio_bands(scheme, bands), stream=stream, ncol=ncol, scheme=scheme, slr=slr or None,
                                                      drbandn=drbandn or None, dfbandn=dfbandn or None, drobio=drobio or None,
                                                      dfobio=dfobio or None))

    def sw_driver_rrtmg_obio_dev(self, stream, ncol, lm, nb_aer, ptr, consts, iceflg, liqflg, sc, dist, isolvar, dyofyr, include_aerosols,
                                 lcldlm, lcldmh, normflx=1, bndsolvar=None, indsolvar=None):
        """sw_driver_rrtmg_dev that also returns the internals DRBANDN / DFBANDN of the ocean-biology coupling (GEOS_SolarGridComp.F90:6385,
        :4148-4151): `ptr` may hold "DRBAND" and "DFBAND" (ncol,14), both or neither (gridcomp.SWD_OBIO_OUT)."""
        self._sw_driver_rrtmg("geosrad_sw_driver_rrtmg_obio_dev", stream, ncol, lm, nb_aer, ptr, consts, iceflg, liqflg, sc, dist, isolvar, dyofyr,
                              include_aerosols, lcldlm, lcldmh, normflx, bndsolvar, indsolvar, **self._obio_out(ptr))

    def sw_driver_rrtmg_obio_lit_dev(self, stream, ncol, nlit, lit_index, lit_pos, lm, nb_aer, ptr, consts, iceflg, liqflg, sc, dist, isolvar,
                                     dyofyr, include_aerosols, lcldlm, lcldmh, normflx=1, bndsolvar=None, indsolvar=None, dark=None, keep=()):
        """sw_driver_rrtmg_lit_dev with "DRBAND" / "DFBAND" as in sw_driver_rrtmg_obio_dev; dark / keep by name over gridcomp.SWD_OUT +
        SWD_OBIO_OUT."""
        obio = self._lit(G.SWD_OBIO_OUT, nlit, 0, 0, dark, [k for k in keep if k in G.SWD_OBIO_OUT])
        self._sw_driver_rrtmg("geosrad_sw_driver_rrtmg_obio_lit_dev", stream, ncol, lm, nb_aer, ptr, consts, iceflg, liqflg, sc, dist, isolvar,
                              dyofyr, include_aerosols, lcldlm, lcldmh, normflx, bndsolvar, indsolvar,
                              **self._lit(G.SWD_OUT, nlit, lit_index, lit_pos, dark, [k for k in keep if k in G.SWD_OUT]),
                              dark_obio=obio["dark"], keep_obio=obio["keep_mask"], **self._obio_out(ptr))

    def rad_tendencies_dev(self, stream, ncol, lm, grav, cp, ptr):
        """heating rates of the parent GridComp (GEOS_RadiationGridComp.F90:798-819)."""
        self._call("geosrad_rad_tendencies_dev", dict(stream=stream, ncol=ncol, lm=lm, grav=grav, cp=cp, **self._io(ptr, G.RT_IN, G.RT_OUT)))

    def profile(self, enable=True):
        self._call("geosrad_profile", {"enable": enable})

    def profile_read(self):
        """{kernel name: (total ms, launches)} measured with HIP events on the launch stream; the names are those of the kernels that ran
        (a rocprofv3 kernel trace of the same run shows them as geosrad::<name><...>)."""
        out = {}
        for k in range(14):
            ms = ctypes.c_double(); n = ctypes.c_long()
            self._call("geosrad_profile_read", {"kernel_id": k, "total_ms": ctypes.byref(ms), "launches": ctypes.byref(n)})
            out[self.L.geosrad_kernel_label(self.h, k).decode()] = (ms.value, n.value)
        return out

    def check(self, stream=0):
        self._call("geosrad_check", {"stream": stream})

    # ---- McICA ---------------------------------------------------------------------------------------------
    def generate_stochastic_clouds(self, ncol, nsubcol, nlay, zmid, alat, doy, play, cldfrac, ciwp, clwp, cwp_tiny,
                                   seed_order=(1, 2, 3, 4)):
        """Inputs in the solver-API layout, numpy (nlay,ncol).  Returns cldy (int32), ciwp_stoch, clwp_stoch as numpy
        (ncol,nsubcol,nlay) == Fortran (nlay,nsubcol,ncol)."""
        a = locals()
        out = dict(self._zeros([("cldy_stoch", (ncol, nsubcol, nlay))], np.int32),
                   **self._zeros([("ciwp_stoch", (ncol, nsubcol, nlay)), ("clwp_stoch", (ncol, nsubcol, nlay))]))
        self._host("geosrad_mcica", a, out, seed_order=(ctypes.c_int32 * 4)(*[int(s) for s in seed_order]))
        return out["cldy_stoch"], out["ciwp_stoch"], out["clwp_stoch"]

    def generate_stochastic_clouds_dev(self, stream, ncol, nsubcol, nlay, ptr, doy, cwp_tiny, seed_order=(1, 2, 3, 4)):
        """device-pointer variant: `ptr` maps zm, alat, play, cldf, ciwp, clwp (inputs, solver-API layout) and
        cldy_stoch (int32), ciwp_stoch, clwp_stoch (outputs, Fortran (nlay,nsubcol,ncol)) to device addresses."""
        self._dev("geosrad_mcica_dev", ptr, _MCICA_PTR, stream=stream, ncol=ncol, nsubcol=nsubcol, nlay=nlay, doy=doy, cwp_tiny=cwp_tiny,
                  seed_order=(ctypes.c_int32 * 4)(*[int(s) for s in seed_order]))

    # ---- lit-column compaction (GEOS_SolarGridComp.F90:3686, PackIt / UnPackIt :7753-7799); device addresses ------------------
    def lit_index_dev(self, stream, ncol, zth, lit_index, lit_pos, nlit_dev, want_count=True):
        """zth: (ncol,) reals; lit_index, lit_pos: (ncol,) int32; nlit_dev: (1,) int32.  Returns NumLit when want_count (synchronises)."""
        n = ctypes.c_int(0)
        self._call("geosrad_lit_index_dev", dict(stream=stream, ncol=ncol, zth=zth, lit_index=lit_index, lit_pos=lit_pos, nlit_dev=nlit_dev,
                                                 nlit_host=ctypes.byref(n) if want_count else None))
        return n.value if want_count else None

    def lit_pack_dev(self, stream, pdim, udim, nlev, lit_index, nlit_dev, unpacked, packed):
        self._call("geosrad_lit_pack_dev", dict(stream=stream, pdim=pdim, udim=udim, nlev=nlev, lit_index=lit_index, nlit_dev=nlit_dev,
                                                unpacked=unpacked, packed=packed))

    def lit_unpack_dev(self, stream, pdim, udim, nlev, lit_pos, packed, unpacked, default=None):
        self._call("geosrad_lit_unpack_dev", dict(stream=stream, pdim=pdim, udim=udim, nlev=nlev, lit_pos=lit_pos, packed=packed,
                                                  unpacked=unpacked, use_default=default is not None, dflt=0.0 if default is None else default))

    def clearCounts_threeBand(self, ncol, nsubcol, nlay, cloudLM, cloudMH, cldy_stoch):
        cnt = np.zeros((ncol, 4), dtype=np.int32)
        self._call("geosrad_clearcounts", dict(ncol=ncol, nsubcol=nsubcol, nlay=nlay, cloudLM=cloudLM, cloudMH=cloudMH,
                                               cldy_stoch=np.ascontiguousarray(cldy_stoch, dtype=np.int32), clearCnts=cnt))
        return cnt


def _obio_bands(scheme, bands):
    """the nbands, wvn1, wvn2, order arguments of geosrad_obio_weights / geosrad_sw_update_obio_dev"""
    if int(scheme) != G.OBIO_BANDS:
        return {"nbands": G.OBIO_NBANDS.get(int(scheme), 0) if bands is None else int(bands), "wvn1": None, "wvn2": None, "order": None}
    w1, w2, od = bands
    return {"nbands": len(w1), "wvn1": _doubles([float(x) for x in w1]), "wvn2": _doubles([float(x) for x in w2]),
            "order": (ctypes.c_int32 * len(od))(*[int(x) for x in od])}


def obio_weights(scheme, real_kind, bands=None):
    """geosrad_obio_weights (no device, no context): the (nbands, 33) array of wavenumber-overlap fractions of the SOLAR TO OBIO conversion
    (GEOS_SolarGridComp.F90:7665-7728), computed in real_kind and widened to float64, and the number of overlaps.  scheme: gridcomp.OBIO_CHOU
    | OBIO_RRTMG | OBIO_BANDS; bands = (wvn1, wvn2, order) in cm-1 / 1-based for OBIO_BANDS (for a built-in scheme an int overrides nbands)."""
    L = _lib.lib()
    vals = _obio_bands(scheme, bands)
    w = np.zeros((max(vals["nbands"], 0), 33), dtype=np.float64)
    npairs = ctypes.c_int32(0)
    rc = L.geosrad_obio_weights(*_args("geosrad_obio_weights", dict(vals, scheme=scheme, real_kind=real_kind, weights=w, npairs=ctypes.byref(npairs))))
    if rc:
        err = GeosradError(L.geosrad_last_error(None).decode())
        err.rc = rc
        raise err
    return w, npairs.value
