"""Shared by the gettau tests: the plain-C restatement of gettau.F90 (tests/gettau_impl.h + gettau_ref.c, compiled into pytest's temporary
directory with -O2 -ffp-contract=off), the synthetic batches and the hand-built columns.

Arrays are numpy C order with the reversed Fortran shape of include/geosrad_gettau.h: cosz (ncol); dp, fcld (nlevs, ncol); reff, hyd
(4, nlevs, ncol); tcldlyr, enn (nlevs + 1, ncol)."""
import ctypes
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
PREC = {4: "f32", 8: "f64"}
GRAV = 9.80665
K_LOG10 = 64            # tests/test_sw_clouds.py: eps of the unscaled thickness that log10 + the cancelling table interpolation may move
HAND_MODES = [(0, 0), (4, 7), (1, 1), (11, 11)]      # in-cloud; three super-layers; high and middle empty; middle and low empty


def build_ref(tmp):
    """the restatement as a loaded library with the oracle's tables set from data/chou_{sw,lw}_r{4,8}.grtb"""
    from geosradiation_gridcomp_amd import _lib
    from geosradiation_gridcomp_amd.tableblob import read_blob
    so = str(tmp / "libgettau.so")
    subprocess.check_call([os.environ.get("CC", "gcc"), "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-std=gnu11", "-w", "-o", so,
                           os.path.join(HERE, "gettau_ref.c"), "-lm"])
    L = ctypes.CDLL(so)
    keep = []                                   # the restatement keeps pointers to the tables
    for kind, sfx in (("r4", "f32"), ("r8", "f64")):
        for blob, setter in (("chou_sw", "oracle_chou_sw_set_table"), ("chou_lw", "oracle_chou_set_table")):
            _, t = read_blob(os.path.join(_lib.DATA, f"{blob}_{kind}.grtb"))
            fn = getattr(L, f"{setter}_{sfx}")
            fn.argtypes = [ctypes.c_char_p, ctypes.c_void_p]
            for name, a in t.items():
                flat = np.ascontiguousarray(np.asfortranarray(a).ravel(order="F"))
                keep.append(flat)
                fn(name.encode(), flat.ctypes.data_as(ctypes.c_void_p))
    return Ref(L, keep)


class Ref:
    def __init__(self, L, keep):
        self.L, self._keep = L, keep

    @staticmethod
    def _in(a, dt):
        x = {k: np.ascontiguousarray(a[k], dtype=dt) for k in ("cosz", "dp", "fcld", "reff", "hyd")}
        nlevs, ncol = x["dp"].shape
        assert x["reff"].shape == x["hyd"].shape == (4, nlevs, ncol) and x["cosz"].shape == (ncol,) and x["fcld"].shape == (nlevs, ncol)
        return x, ncol, nlevs

    def _run(self, name, rk, args):
        R = ctypes.c_float if rk == 4 else ctypes.c_double
        conv = [a.ctypes.data_as(ctypes.c_void_p) if isinstance(a, np.ndarray) else R(a) if isinstance(a, float) else ctypes.c_int(a) for a in args]
        assert getattr(self.L, f"{name}_{PREC[rk]}")(*conv) == 0

    def swtau(self, ib, a, ict, icb, rk, grav=GRAV):
        """getvistau.code (ib = 0) / getnirtau.code (ib = 1..3): taubeam, taudiff (4, nlevs, ncol), asycl, ssacl (nlevs, ncol)"""
        dt = np.float32 if rk == 4 else np.float64
        x, ncol, nlevs = self._in(a, dt)
        o = {"taubeam": np.zeros((4, nlevs, ncol), dt), "taudiff": np.zeros((4, nlevs, ncol), dt), "asycl": np.zeros((nlevs, ncol), dt),
             "ssacl": np.zeros((nlevs, ncol), dt)}
        self._run("gtr_swtau", rk, [ib, ncol, nlevs, x["cosz"], x["dp"], x["fcld"], x["reff"], x["hyd"], ict, icb, float(grav), o["taubeam"],
                                   o["taudiff"], o["asycl"], o["ssacl"]])
        if ib == 0:
            del o["ssacl"]
        return o

    def irtau(self, ib, a, rk, grav=GRAV):
        """getirtau.code: taudiag (4, nlevs, ncol), tcldlyr, enn (nlevs + 1, ncol)"""
        dt = np.float32 if rk == 4 else np.float64
        x, ncol, nlevs = self._in(a, dt)
        o = {"taudiag": np.zeros((4, nlevs, ncol), dt), "tcldlyr": np.zeros((nlevs + 1, ncol), dt), "enn": np.zeros((nlevs + 1, ncol), dt)}
        self._run("gtr_irtau", rk, [ib, ncol, nlevs, x["dp"], x["fcld"], x["reff"], x["hyd"], float(grav), o["taudiag"], o["tcldlyr"], o["enn"]])
        return o

    def oracle_swtau(self, ib, a, ict, icb, rk):
        """the oracle's cs_gettau column by column: the species SUMS tauclb, tauclf and asycl, ssacl (nlevs, ncol)"""
        dt = np.float32 if rk == 4 else np.float64
        x, ncol, nlevs = self._in(a, dt)
        o = {k: np.zeros((nlevs, ncol), dt) for k in ("tauclb", "tauclf", "asycl", "ssacl")}
        self._run("gtr_oracle_swtau", rk, [ib, ncol, nlevs, x["cosz"], x["dp"], x["fcld"], x["reff"], x["hyd"], ict, icb, o["tauclb"], o["tauclf"],
                                          o["asycl"], o["ssacl"]])
        return o

    def oracle_irtau(self, ib, a, rk):
        """the oracle's ch_getirtau column by column"""
        dt = np.float32 if rk == 4 else np.float64
        x, ncol, nlevs = self._in(a, dt)
        o = {"taudiag": np.zeros((4, nlevs, ncol), dt), "tcldlyr": np.zeros((nlevs + 1, ncol), dt), "enn": np.zeros((nlevs + 1, ncol), dt)}
        self._run("gtr_oracle_irtau", rk, [ib, ncol, nlevs, x["dp"], x["fcld"], x["reff"], x["hyd"], o["taudiag"], o["tcldlyr"], o["enn"]])
        return o

    def lw_cloud_diag(self, f, rk, taucrit=0.30, grav=GRAV, undef=1.0e15):
        """TAUIR (lm, ncol), CLDTMP, CLDPRS (ncol) from the GEOS fields f (PLE (lm + 1, ncol); T, QI .. RS (lm, ncol))"""
        dt = np.float32 if rk == 4 else np.float64
        x = {k: np.ascontiguousarray(f[k], dtype=dt) for k in ("PLE", "T", "QI", "QL", "QR", "QS", "RI", "RL", "RR", "RS")}
        lm, ncol = x["T"].shape
        q = (ctypes.c_void_p * 4)(*[x[k].ctypes.data for k in ("QI", "QL", "QR", "QS")])
        r = (ctypes.c_void_p * 4)(*[x[k].ctypes.data for k in ("RI", "RL", "RR", "RS")])
        o = {"TAUIR": np.zeros((lm, ncol), dt), "CLDTMP": np.zeros(ncol, dt), "CLDPRS": np.zeros(ncol, dt)}
        R = ctypes.c_float if rk == 4 else ctypes.c_double
        p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
        assert getattr(self.L, f"gtr_lw_cloud_diag_{PREC[rk]}")(ctypes.c_int(ncol), ctypes.c_int(lm), R(grav), R(undef), R(taucrit), p(x["PLE"]),
                                                               p(x["T"]), q, r, p(o["TAUIR"]), p(o["CLDTMP"]), p(o["CLDPRS"])) == 0
        return o


def synth_batch(ncol, nlevs, start=9100, lw=False):
    """(inputs, LCLDMH, LCLDLM) from synth.make_columns.  For getvistau / getnirtau through synth.geos_chou_sw_fields: the Solar GridComp's own
    preparation (REFF = R * 1.e6 with MAPL_UNDEF radii in every 7th cell, i.e. 1e21 microns and a negligible thickness,
    GEOS_SolarGridComp.F90:7238-7249).  lw: for getirtau, the arguments irrad hands it (synth.chou_lw_inputs; the Irrad GridComp replaces
    undefined radii before the call, so there are none - 1e21 microns would overflow getirtau's cubic polynomials in fp32).
    nlevs < 4: the lowest layers of a 4-layer batch."""
    from geosradiation_gridcomp_amd import synth
    nl = max(nlevs, 4)
    inp = synth.make_columns(ncol, nl, start=start, cloudy_frac=0.7, aerosol=False)
    if lw:
        c = synth.chou_lw_inputs(inp)
        a = {"cosz": np.zeros(ncol), "dp": np.diff(c["ple"].astype(np.float64), axis=0)[nl - nlevs:], "fcld": c["fcld"][nl - nlevs:],
             "reff": c["reff"][:, nl - nlevs:], "hyd": c["cwc"][:, nl - nlevs:]}
        ict, icb = int(c["ict"]), int(c["icb"])
    else:
        s = synth.geos_chou_sw_fields(inp, aerosol=False)
        a = {"cosz": s["ZT"], "dp": np.diff(s["PLE"], axis=0)[nl - nlevs:], "fcld": s["CL"][nl - nlevs:],
             "reff": np.stack([s[k] * 1.0e6 for k in ("RI", "RL", "RR", "RS")])[:, nl - nlevs:],
             "hyd": np.stack([s[k] for k in ("QI", "QL", "QR", "QS")])[:, nl - nlevs:]}
        ict, icb = int(s["LCLDMH"]), int(s["LCLDLM"])
    return {k: np.ascontiguousarray(v, dtype=np.float64) for k, v in a.items()}, min(ict, nlevs + 1), min(icb, nlevs + 1)


def hand_columns(ref):
    """ten hand-built columns of 10 layers (float64) for the super-layers 1-3 / 4-6 / 7-10 of mode (4, 7):
      0 cloudy in all three super-layers                    1 reff <= 0 in each species, layer by layer
      2 snow radius 80 / 112 / 140 / 1000 microns           3 liquid only, tauc (UV/PAR) = 0.0199, 0.0201, 0.5, 31, 33, 40 ...
      4 fcld = 0.005, 0.011, 1 under heavy condensate       5 every layer at its super-layer's maximum cover (ia clamps at 10)
      6 = 0 with cosz = 0.01 (im clamps at 2)               7 = 0 with cosz = 1.0 (im clamps at 10)
      8 cover but no condensate                             9 condensate, but no cover in the middle super-layer"""
    lm, n = 10, 10
    a = {"cosz": np.full(n, 0.6), "dp": np.linspace(2000.0, 12000.0, lm)[:, None] * np.ones(n)}
    fc = np.array([0.0, 0.3, 0.5, 0.2, 0.6, 0.1, 0.8, 0.4, 0.0, 0.9])
    a["fcld"] = np.repeat(fc[:, None], n, axis=1)
    a["hyd"] = np.stack([np.full((lm, n), v) for v in (2e-5, 1e-4, 3e-5, 4e-5)])
    a["reff"] = np.stack([np.full((lm, n), v) for v in (30.0, 12.0, 100.0, 80.0)])
    for l, s in enumerate((0, 1, 3, 2, 0, 1, 3)):          # column 1: one species' radius <= 0 per layer (rain's does not enter)
        a["reff"][s, l + 1, 1] = 0.0 if l % 2 == 0 else -5.0
    a["reff"][:, 9, 1] = 0.0
    a["reff"][3, :, 2] = np.array([80.0, 112.0, 140.0, 1000.0, 111.99, 112.01, 80.0, 140.0, 112.0, 500.0])
    a["hyd"][:, :, 3] = 0.0
    a["hyd"][1, :, 3] = 1.0
    a["fcld"][:, 3] = 0.7
    unit = ref.swtau(0, {k: v[..., 3:4] for k, v in a.items()}, 0, 0, 8)["taudiff"][1, :, 0]       # tauc per unit liquid mixing ratio
    a["hyd"][1, :, 3] = np.array([0.0199, 0.0201, 0.5, 31.0, 33.0, 40.0, 0.019, 0.021, 2.0, 100.0]) / unit
    a["hyd"][:, :, 4] *= 20.0
    a["fcld"][:, 4] = np.array([0.005, 0.011, 1.0, 0.005, 0.011, 1.0, 0.005, 0.011, 1.0, 0.0101])
    a["fcld"][:, 5] = np.array([0.3, 0.3, 0.3, 0.6, 0.6, 0.6, 0.9, 0.9, 0.9, 0.9])
    a["cosz"][6], a["cosz"][7] = 0.01, 1.0
    a["hyd"][:, :, 8] = 0.0
    a["fcld"][3:6, 9] = 0.0
    return {k: np.ascontiguousarray(v, dtype=np.float64) for k, v in a.items()}


def unscaled(ref, ib, a, rk, ir=False):
    """|tc_s|: the species' optical thicknesses before the overlap scaling (the in-cloud mode of the restatement), float64"""
    o = ref.irtau(ib, a, rk)["taudiag"] if ir else ref.swtau(ib, a, 0, 0, rk)["taudiff"]
    return np.abs(o.astype(np.float64))


def ulp(a, b):
    a64, b64 = a.astype(np.float64), b.astype(np.float64)
    sp = np.spacing(np.maximum(np.abs(a), np.abs(b)).astype(a.dtype)).astype(np.float64)
    return np.where(a64 == b64, 0.0, np.abs(a64 - b64) / sp)
