"""Cloud diagnostics of the Solar GridComp's UPDATE_EXPORT on the device (geosrad_sw_update_clouds_dev / Context.sw_update_clouds_dev):
GEOS_SolarGridComp.F90:7006-7058 (super-layer cloud fractions) and :7223-7392 (GETVISTAU per column, optical thicknesses, cloud top).

The numbers are checked against a plain-C restatement (tests/sw_clouds_impl.h) compiled here into pytest's temporary directory with
-O2 -ffp-contract=off.  It keeps GETVISTAU's taudiff per species; its species sum is checked bit for bit against the oracle's own
getvistau (cs_gettau), an independent statement of the same routine.

The optical thicknesses go through log10 (getvistau.code's table abscissa).  The device's log10 and glibc's are each accurate to a few
ulp, not correctly rounded, and GETVISTAU's scaling factor (xai = ... - caif(it,ia), a cancellation) carries such a difference into tens
of ulp of a small result (measured on the MI355X: up to 47 ulp in fp32, 23 in fp64).  xai lies in [0, 1] and its error is absolute, so
these exports are held to K_LOG10 eps of the UNSCALED optical thickness they are made from (tc_s of getvistau.code, computed here from
the inputs), plus 2 ulp; the tests report how many cells differ at all and by more than 2 ulp.
The cloud fractions are bitwise; the cloud top is exact except next to taucrit."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from tests.conftest import ROOT

HERE = os.path.dirname(os.path.abspath(__file__))
PREC = {4: "f32", 8: "f64"}
EXACT = ["FCLD_X", "CLDLO", "CLDMD", "CLDHI", "CLDTT", "COTDENLO", "COTDENMD", "COTDENHI", "COTDENTT"]
TAUCRIT = 0.10
K_LOG10 = 64


# ---- the restatement -----------------------------------------------------------------------------------------------------------------
class _Ref:
    def __init__(self, L, keep):
        self.L, self._keep = L, keep

    def clouds(self, f, lcldmh, lcldlm, dt, taucrit=TAUCRIT, grav=9.80665, undef=1.0e15):
        """every export of the cloud block for fields f (gridcomp.SWK_IN names, (LM[+1], ncol) arrays of dtype dt)"""
        from geosradiation_gridcomp_amd import gridcomp as G
        lm, ncol = f["FCLD"].shape
        ins = [np.ascontiguousarray(f[k], dtype=dt) for k in G.SWK_IN]
        outs = {k: np.full((lm, ncol) if k in G.SWK_OUT_3D else (ncol,), -7.0, dtype=dt) for k in G.SWK_OUT}
        pin = (ctypes.c_void_p * len(ins))(*[a.ctypes.data for a in ins])
        pout = (ctypes.c_void_p * len(outs))(*[outs[k].ctypes.data for k in G.SWK_OUT])
        R = ctypes.c_float if dt == np.float32 else ctypes.c_double
        fn = getattr(self.L, "swk_update_clouds_" + PREC[np.dtype(dt).itemsize])
        assert fn(ctypes.c_int(ncol), ctypes.c_int(lm), ctypes.c_int(lcldmh), ctypes.c_int(lcldlm), R(taucrit), R(grav), R(undef), pin, pout) == 0
        return outs

    def column_sums(self, name, rk, cosz, dp, fcld, reff, hyd, ict, icb):
        """swk_getvistau_sum / swk_cs_tauclf on one column: 1-based (np+1) arrays, reff / hyd (4, np+1)"""
        dt = np.float32 if rk == 4 else np.float64
        R = ctypes.c_float if rk == 4 else ctypes.c_double
        a = [np.ascontiguousarray(x, dtype=dt) for x in (dp, fcld, reff, hyd)]
        out = np.zeros(a[0].shape[0], dtype=dt)
        p = lambda x: x.ctypes.data_as(ctypes.c_void_p)
        args = [ctypes.c_int(a[0].shape[0] - 1), R(cosz)] + [p(x) for x in a] + [ctypes.c_int(ict), ctypes.c_int(icb)]
        if name == "swk_getvistau_sum":
            args.append(R(9.80665))
        assert getattr(self.L, f"{name}_{PREC[rk]}")(*args, p(out)) == 0
        return out[1:]


@pytest.fixture(scope="session")
def swkref(tmp_path_factory):
    from geosradiation_gridcomp_amd import _lib
    from geosradiation_gridcomp_amd.tableblob import read_blob
    so = str(tmp_path_factory.mktemp("sw_clouds") / "libsw_clouds.so")
    subprocess.check_call([os.environ.get("CC", "gcc"), "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-std=gnu11", "-w", "-o", so,
                           os.path.join(HERE, "sw_clouds_ref.c"), "-lm"])
    L = ctypes.CDLL(so)
    keep = []                                   # the restatement keeps pointers to the tables
    for kind, sfx in (("r4", "f32"), ("r8", "f64")):
        _, t = read_blob(os.path.join(_lib.DATA, f"chou_sw_{kind}.grtb"))
        fn = getattr(L, f"oracle_chou_sw_set_table_{sfx}")
        fn.argtypes = [ctypes.c_char_p, ctypes.c_void_p]
        for name, a in t.items():
            flat = np.ascontiguousarray(np.asfortranarray(a).ravel(order="F"))
            keep.append(flat)
            fn(name.encode(), flat.ctypes.data_as(ctypes.c_void_p))
    return _Ref(L, keep)


# ---- inputs --------------------------------------------------------------------------------------------------------------------------
def _fields(ncol, lm=72, start=3100, seed=5, night=0.4, clear=0.1):
    """GEOS-side imports (gridcomp.SWK_IN, (LM[+1], ncol) float64) from synth.geos_chou_sw_fields: MAPL_UNDEF radii in every 7th
    cell, ZTH < 0 in a `night` share of the columns, a `clear` share of the columns without any cloud; plus LCLDMH / LCLDLM"""
    from geosradiation_gridcomp_amd import synth
    inp = synth.make_columns(ncol, lm, start=start, cloudy_frac=0.7, aerosol=False)
    s = synth.geos_chou_sw_fields(inp, aerosol=False)
    rng = np.random.default_rng(seed)
    f = {"FCLD": s["CL"].copy(), "PLE": s["PLE"], "T": s["T"], "ZTH": s["ZT"].copy()}
    for k in ("QI", "QL", "QR", "QS", "RI", "RL", "RR", "RS"):
        f[k] = s[k]
    f["ZTH"][rng.uniform(0, 1, ncol) < night] *= -0.5
    f["FCLD"][:, rng.uniform(0, 1, ncol) < clear] = 0.0
    return f, int(s["LCLDMH"]), int(s["LCLDLM"])


def _hand_columns(dt):
    """eight hand-built columns of 10 layers, super-layers 1-3 / 4-6 / 7-10 (lcldmh = 4, lcldlm = 7):
      0 cloudy in all three super-layers       1 only the middle super-layer cloudy     2 all clear (condensate, no cover)
      3 = 0 with RI and RS MAPL_UNDEF          4 = 3 with RS = 1 mm (capped at 112 um, like the undefined one)
      5 = 0 as a night column (ZTH < 0)        6 = 0 with ZTH = 0                       7 = 0 with no condensate above layer 5"""
    lm, n = 10, 8
    ple = np.linspace(1000.0, 100000.0, lm + 1)[:, None] * np.ones(n)
    f = {"PLE": ple, "T": np.linspace(210.0, 290.0, lm)[:, None] + np.arange(n)[None, :] * 0.5, "ZTH": np.full(n, 0.6)}
    fc = np.array([0.0, 0.3, 0.5, 0.2, 0.6, 0.1, 0.8, 0.4, 0.0, 0.9])
    f["FCLD"] = np.repeat(fc[:, None], n, axis=1)
    f["FCLD"][:, 1] = np.where((np.arange(lm) >= 3) & (np.arange(lm) < 6), fc, 0.0)
    f["FCLD"][:, 2] = 0.0
    for q, v in (("QI", 2e-5), ("QL", 1e-4), ("QR", 3e-5), ("QS", 4e-5)):
        f[q] = np.full((lm, n), v)
    for q in ("QI", "QL", "QR", "QS"):
        f[q][:, 7] = np.where(np.arange(lm) >= 5, 1e-4, 0.0)
    for r, v in (("RI", 30e-6), ("RL", 12e-6), ("RR", 100e-6), ("RS", 80e-6)):
        f[r] = np.full((lm, n), v)
    f["RI"][:, 3] = f["RI"][:, 4] = 1.0e15
    f["RS"][:, 3] = 1.0e15
    f["RS"][:, 4] = 1.0e-3
    f["ZTH"][5] = -0.4
    f["ZTH"][6] = 0.0
    return {k: np.ascontiguousarray(v, dtype=dt) for k, v in f.items()}, 4, 7


def _ulp(a, b):
    a64, b64 = a.astype(np.float64), b.astype(np.float64)
    sp = np.spacing(np.maximum(np.abs(a), np.abs(b)).astype(a.dtype)).astype(np.float64)
    return np.where(a64 == b64, 0.0, np.abs(a64 - b64) / sp)


# ---- CPU -----------------------------------------------------------------------------------------------------------------------------
def test_symbol_exported():
    from geosradiation_gridcomp_amd import _lib
    assert "geosrad_sw_update_clouds_dev" in _lib.EXPORTS
    L = _lib.lib()
    assert hasattr(L, "geosrad_sw_update_clouds_dev")
    assert L.geosrad_sw_update_clouds_dev(None, None, 1, 10, 4, 7, ctypes.c_double(0.1), None, None, None) == 1     # EINVAL, null context


def test_header_orders_match_gridcomp_lists():
    from geosradiation_gridcomp_amd import gridcomp as G
    h = open(os.path.join(ROOT, "include", "geosrad.h")).read()
    enums = [re.findall(r"GEOSRAD_SWK_(\w+)", e) for e in re.findall(r"enum\s*\{([^}]*GEOSRAD_SWK_[^}]*)\}", h)]
    assert len(enums) == 3
    ins, consts, outs = enums
    assert ins[-1] == "NIN" and ins[:-1] == G.SWK_IN
    assert consts[-1] == "NCONST" and [c[2:] for c in consts[:-1]] == G.SWK_CONST
    assert outs[-1] == "NOUT" and outs[:-1] == G.SWK_OUT
    assert len(G.swk_consts()) == len(G.SWK_CONST)
    F = open(os.path.join(ROOT, "geosradiation_gridcomp_amd", "fortran", "gridcomp_shims.F90")).read()
    for names, pre in ((G.SWK_IN, "SWK_"), (G.SWK_OUT, "SWK_")):
        for i, k in enumerate(names):
            assert re.search(rf"\b{pre}{k}\s*=\s*{i + 1}\b", F), k


@pytest.mark.parametrize("rk", [4, 8])
def test_restatement_species_sum_equals_oracle_getvistau(swkref, rk):
    """the restatement's per-species taudiff, summed as SOL:7280 sums it, is the oracle's tauclf (cs_gettau, ib = 0) bit for bit"""
    dt = np.float32 if rk == 4 else np.float64
    f, ict, icb = _fields(96, start=777, seed=3)
    f = {k: v.astype(dt) for k, v in f.items()}
    lm = f["FCLD"].shape[0]
    cloudy = 0
    for i in range(f["FCLD"].shape[1]):
        one = lambda a: np.concatenate([[0], a[:, i]]).astype(dt)
        dp = one(f["PLE"][1:] - f["PLE"][:-1])
        reff = np.stack([one(f[r]) * dt(1.e6) for r in ("RI", "RL", "RR", "RS")])
        hyd = np.stack([one(f[q]) for q in ("QI", "QL", "QR", "QS")])
        cosz = max(float(f["ZTH"][i]), 0.0)
        a = swkref.column_sums("swk_getvistau_sum", rk, cosz, dp, one(f["FCLD"]), reff, hyd, ict, icb)
        b = swkref.column_sums("swk_cs_tauclf", rk, cosz, dp, one(f["FCLD"]), reff, hyd, ict, icb)
        np.testing.assert_array_equal(a, b)
        cloudy += int((a > 0).sum())
        assert a.shape == (lm,)
    assert cloudy > 150


@pytest.mark.parametrize("rk", [4, 8])
def test_restatement_edge_rules_on_hand_built_columns(swkref, rk):
    dt = np.float32 if rk == 4 else np.float64
    f, mh, ml = _hand_columns(dt)
    ud = dt(1.0e15)
    o = swkref.clouds(f, mh, ml, dt)
    tot = o["TAUCLI"] + o["TAUCLW"] + o["TAUCLR"] + o["TAUCLS"]
    # super-layers: column 1 has cloud in the middle one only; column 2 is clear
    assert o["CLDHI"][1] == 0 and o["CLDLO"][1] == 0 and o["CLDMD"][1] == dt(0.6) and o["CLDTT"][1] == o["CLDMD"][1]
    assert o["COTHI"][1] == ud and o["COTLO"][1] == ud and o["COTMD"][1] == o["TAUMD"][1] > 0
    assert o["TAUHI"][1] == 0 and o["TAULO"][1] == 0 and o["COTNUMHI"][1] == 0
    np.testing.assert_allclose(o["TAUTX"][1], o["TAUMD"][1], rtol=4 * np.finfo(dt).eps)
    for k in ("CLDLO", "CLDMD", "CLDHI", "CLDTT", "TAULO", "TAUMD", "TAUHI", "TAUTT", "TAUTX", "COTNUMLO", "COTNUMTT"):
        assert o[k][2] == 0, k
    for k in ("COTLO", "COTMD", "COTHI", "COTTT", "CLDTMP", "CLDPRS"):
        assert o[k][2] == ud, k
    assert (tot[:, 2] == 0).all()
    # super-layer sums top down, TAUTT, TAUTX, COTNUM
    c0 = tot[:, 0]
    assert o["TAUHI"][0] == (dt(0) + c0[0] + c0[1] + c0[2]) and o["TAULO"][0] == (((dt(0) + c0[6]) + c0[7]) + c0[8]) + c0[9]
    assert o["TAUTT"][0] == (o["TAUHI"][0] + o["TAUMD"][0]) + o["TAULO"][0]
    assert o["TAUTX"][0] == ((o["TAULO"][0] * o["CLDLO"][0] + o["TAUMD"][0] * o["CLDMD"][0]) + o["TAUHI"][0] * o["CLDHI"][0]) / o["CLDTT"][0]
    assert o["CLDTT"][0] == dt(1) - ((dt(1) - o["CLDHI"][0]) * (dt(1) - o["CLDMD"][0])) * (dt(1) - o["CLDLO"][0])
    assert o["COTNUMTT"][0] == o["CLDTT"][0] * o["TAUTX"][0] and o["COTTT"][0] == o["TAUTX"][0]
    # no cover, no optical thickness: layer 1 (fcld 0) and layer 9 (fcld 0) of column 0
    assert tot[0, 0] == 0 and tot[8, 0] == 0 and (tot[[1, 2, 3, 4, 6, 7, 9], 0] > 0).all()
    # undefined radii: 1e21 um, a negligible thickness; snow capped at 112 um like a 1 mm radius
    for k in ("TAUCLI", "TAUCLW", "TAUCLR", "TAUCLS"):
        assert (o[k][:, 3] == o[k][:, 4]).all(), k
    assert (o["TAUCLS"][:, 3] > 0).sum() > 3 and (o["TAUCLW"][:, 3] > 0).sum() > 3 and (o["TAUCLI"][:, 3] < 1e-12).all()
    # the night column and ZTH = 0 give column 0's optical thicknesses (GETVISTAU's taudiff does not depend on cosz)
    for k in ("TAUCLI", "TAUCLW", "TAUCLR", "TAUCLS"):
        assert (o[k][:, 5] == o[k][:, 0]).all() and (o[k][:, 6] == o[k][:, 0]).all(), k
    # cloud top: the topmost layer with total > taucrit; column 7's condensate starts at layer 6
    k0 = int(np.argmax(tot[:, 0] > dt(TAUCRIT)))
    assert o["CLDTMP"][0] == f["T"][k0, 0] and o["CLDPRS"][0] == f["PLE"][k0, 0]
    assert o["CLDPRS"][7] == f["PLE"][5, 7] and o["CLDTMP"][7] == f["T"][5, 7]
    # a layer whose total equals taucrit exactly does not count (strict >): the next one down becomes the top
    o2 = swkref.clouds(f, mh, ml, dt, taucrit=float(tot[k0, 0]))
    k1 = k0 + 1 + int(np.argmax(tot[k0 + 1:, 0] > tot[k0, 0]))
    assert tot[k1, 0] > tot[k0, 0] and o2["CLDTMP"][0] == f["T"][k1, 0] and o2["CLDPRS"][0] == f["PLE"][k1, 0]


@pytest.mark.parametrize("rk", [4, 8])
def test_restatement_passes_the_self_consistency_check(swkref, rk):
    """_self_consistent (the bitwise statement-order check the GPU tests apply to the kernel) holds for the restatement itself"""
    dt = np.float32 if rk == 4 else np.float64
    f, mh, ml = _fields(400, start=2100, seed=4)
    f = {k: v.astype(dt) for k, v in f.items()}
    _self_consistent(swkref.clouds(f, mh, ml, dt), f, mh, ml, dt)
    h, hmh, hml = _hand_columns(dt)
    _self_consistent(swkref.clouds(h, hmh, hml, dt), h, hmh, hml, dt)


# ---- GPU -----------------------------------------------------------------------------------------------------------------------------
def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def _run(ctx, f, mh, ml, names=None, taucrit=TAUCRIT, sentinel=-7.0, drop=()):
    """the device entry point on fields f; exports `names` (default all), every other export allocated, sentinel-filled, not passed"""
    import torch
    from geosradiation_gridcomp_amd import gridcomp as G
    dt = ctx.dtype
    lm, ncol = f["FCLD"].shape
    t = {k: torch.from_numpy(np.ascontiguousarray(f[k], dtype=dt)).cuda() for k in G.SWK_IN if k not in drop}
    tdt = torch.float32 if dt == np.float32 else torch.float64
    o = {k: torch.full((lm, ncol) if k in G.SWK_OUT_3D else (ncol,), sentinel, dtype=tdt, device="cuda") for k in G.SWK_OUT}
    names = G.SWK_OUT if names is None else names
    ptr = {k: v.data_ptr() for k, v in t.items()}
    ptr.update({k: o[k].data_ptr() for k in names})
    try:
        ctx.sw_update_clouds_dev(_stream(), ncol, lm, mh, ml, taucrit, ptr, consts=[9.80665, float(dt(1.0e15))])
    finally:
        torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in o.items()}


def _unscaled(f, dt):
    """|tc_s| of getvistau.code (the species' optical thickness before the cover scaling), (4, LM, ncol), in precision dt"""
    from geosradiation_gridcomp_amd import _lib
    from geosradiation_gridcomp_amd.tableblob import read_blob
    _, t = read_blob(os.path.join(_lib.DATA, f"chou_sw_{'r4' if dt == np.float32 else 'r8'}.grtb"))
    aib, awb, arb = dt(np.ravel(t["aib_uv"])[0]), np.ravel(t["awb_uv"]).astype(dt), np.ravel(t["arb_uv"]).astype(dt)
    wp = ((f["PLE"][1:] - f["PLE"][:-1]).astype(dt) * dt(1.0e3)) / dt(9.80665)
    r = [f[k].astype(dt) * dt(1.e6) for k in ("RI", "RL", "RR", "RS")]
    q = [f[k].astype(dt) for k in ("QI", "QL", "QR", "QS")]
    rs = np.minimum(r[3], dt(112.0))
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        tc = [np.where(r[0] <= 0, 0, (wp * q[0]) * aib / r[0]), np.where(r[1] <= 0, 0, (wp * q[1]) * (awb[0] + awb[1] / r[1])),
              (wp * q[2]) * arb[0], np.where(rs <= 0, 0, (wp * q[3]) * aib / rs)]
    return np.abs(np.stack(tc).astype(np.float64))


def _compare(got, swkref, f, mh, ml, dt, taucrit=TAUCRIT, report=""):
    """bitwise for the cloud fractions; within K_LOG10 eps of the unscaled optical thickness (module docstring) for what goes through
    log10; the cloud top exact except where a layer total lies within that bound of taucrit"""
    from geosradiation_gridcomp_amd import gridcomp as G
    ref = swkref.clouds(f, mh, ml, dt, taucrit=taucrit)
    eps = float(np.finfo(dt).eps)
    tc = _unscaled(f, dt)
    bound = {k: K_LOG10 * eps * tc[s] for s, k in enumerate(("TAUCLI", "TAUCLW", "TAUCLR", "TAUCLS"))}
    col = 3 * K_LOG10 * eps * tc.sum(axis=(0, 1))      # a super-layer sum, TAUTX (<= 3 x the largest), x a fraction <= 1
    for k in EXACT:
        np.testing.assert_array_equal(got[k], ref[k], err_msg=k)
    ndiff, nfar, worst = {}, {}, 0.0
    d64 = lambda a, b: np.abs(a.astype(np.float64) - b.astype(np.float64))
    for k in G.SWK_OUT:
        if k in EXACT or k in ("CLDTMP", "CLDPRS"):
            continue
        u = _ulp(got[k], ref[k])
        ndiff[k], nfar[k] = int((u > 0).sum()), int((u > 2).sum())
        worst = max(worst, float(u.max()))
        ok = d64(got[k], ref[k]) <= bound.get(k, col) + 2 * np.spacing(np.abs(ref[k])).astype(np.float64)
        assert ok.all(), (k, int((~ok).sum()), float(u[~ok].max()))
    t0 = (ref["TAUCLI"] + ref["TAUCLW"] + ref["TAUCLR"] + ref["TAUCLS"]).astype(np.float64)
    near = (np.abs(t0 - float(dt(taucrit))) <= K_LOG10 * eps * tc.sum(axis=0) + 8 * float(np.spacing(dt(taucrit)))).any(axis=0)
    for k in ("CLDTMP", "CLDPRS"):
        bad = got[k] != ref[k]
        assert not (bad & ~near).any(), k
    assert near.mean() < 0.01
    print(f"{report}: cells differing from the restatement: { {k: v for k, v in ndiff.items() if v} or 'none'}; by more than 2 ulp: "
          f"{ {k: v for k, v in nfar.items() if v} or 'none'} (worst {worst:g} ulp); columns with a layer total next to taucrit: "
          f"{int(near.sum())}, cloud tops that differ: {int((got['CLDTMP'] != ref['CLDTMP']).sum())}")
    return ref


def _self_consistent(o, f, mh, ml, dt, taucrit=TAUCRIT, undef=1.0e15):
    """the kernel's exports against each other, bitwise and independent of log10: the statement order of SOL:7280-7388 - the species
    sum ((I + W) + R) + S, the super-layer sums top down, TAUTT = (HI + MD) + LO, TAUTX = ((LO CLDLO + MD CLDMD) + HI CLDHI) / CLDTT,
    COT / COTNUM, and the cloud top at the topmost layer whose total exceeds taucrit"""
    ud, lm = dt(undef), o["TAUCLI"].shape[0]
    tot = ((o["TAUCLI"] + o["TAUCLW"]) + o["TAUCLR"]) + o["TAUCLS"]
    for name, (a, b) in (("TAUHI", (0, mh - 1)), ("TAUMD", (mh - 1, ml - 1)), ("TAULO", (ml - 1, lm))):
        acc = np.zeros(tot.shape[1], dtype=dt)
        for l in range(a, b):
            acc = acc + tot[l]
        np.testing.assert_array_equal(o[name], acc, err_msg=name)
    th, tm, tl = o["TAUHI"], o["TAUMD"], o["TAULO"]
    ch, cm, cl, ct = o["CLDHI"], o["CLDMD"], o["CLDLO"], o["CLDTT"]
    np.testing.assert_array_equal(ct, dt(1.) - ((dt(1) - ch) * (dt(1) - cm)) * (dt(1) - cl), err_msg="CLDTT")
    np.testing.assert_array_equal(o["TAUTT"], (th + tm) + tl, err_msg="TAUTT")
    tx = np.where(ct > 0, ((tl * cl + tm * cm) + th * ch) / np.where(ct > 0, ct, dt(1)), dt(0)).astype(dt)
    np.testing.assert_array_equal(o["TAUTX"], tx, err_msg="TAUTX")
    for sfx, c, t in (("LO", cl, tl), ("MD", cm, tm), ("HI", ch, th), ("TT", ct, tx)):
        np.testing.assert_array_equal(o["COTNUM" + sfx], c * t, err_msg="COTNUM" + sfx)
        np.testing.assert_array_equal(o["COT" + sfx], np.where(c > 0, t, ud), err_msg="COT" + sfx)
    hit = tot > dt(taucrit)
    k = np.argmax(hit, axis=0)
    cols = np.arange(tot.shape[1])
    np.testing.assert_array_equal(o["CLDTMP"], np.where(hit.any(axis=0), f["T"].astype(dt)[k, cols], ud), err_msg="CLDTMP")
    np.testing.assert_array_equal(o["CLDPRS"], np.where(hit.any(axis=0), f["PLE"].astype(dt)[k, cols], ud), err_msg="CLDPRS")


@pytest.mark.gpu
@pytest.mark.parametrize("rk", [4, 8])
def test_kernel_matches_restatement(gpu_ctx, swkref, rk, capsys):
    """~3 000 columns (a ragged last 256-column block), 40 % night columns, MAPL_UNDEF radii, clear columns, LCLDMH / LCLDLM of the
    synthetic fields; plus the hand-built columns of the edge-rule test"""
    ctx = gpu_ctx[rk]; dt = ctx.dtype
    f, mh, ml = _fields(3000)
    f = {k: v.astype(dt) for k, v in f.items()}
    assert f["FCLD"].shape[1] % 256 != 0 and (f["ZTH"] < 0).mean() > 0.3 and (f["FCLD"].max(axis=0) == 0).sum() > 100
    got = _run(ctx, f, mh, ml)
    with capsys.disabled():
        ref = _compare(got, swkref, f, mh, ml, dt, report=f"r{rk} 3000x72")
    _self_consistent(got, f, mh, ml, dt)
    assert (ref["CLDTMP"] != dt(1e15)).mean() > 0.3 and (ref["COTLO"] == dt(1e15)).any() and (ref["TAUCLS"] > 0).any()
    h, hmh, hml = _hand_columns(dt)
    got = _run(ctx, h, hmh, hml)
    with capsys.disabled():
        _compare(got, swkref, h, hmh, hml, dt, report=f"r{rk} hand-built")
    _self_consistent(got, h, hmh, hml, dt)


@pytest.mark.gpu
@pytest.mark.parametrize("rk", [4, 8])
def test_each_export_alone_gives_the_same_bits(gpu_ctx, rk):
    from geosradiation_gridcomp_amd import gridcomp as G
    ctx = gpu_ctx[rk]
    f, mh, ml = _fields(700, start=4100, seed=9)
    f = {k: v.astype(ctx.dtype) for k, v in f.items()}
    full = _run(ctx, f, mh, ml)
    for k in G.SWK_OUT:
        one = _run(ctx, f, mh, ml, names=[k])
        np.testing.assert_array_equal(one[k], full[k], err_msg=k)
        for j in G.SWK_OUT:
            if j != k:
                assert (one[j] == -7.0).all(), (k, j)
    # ZTH enters no export: it may be NULL
    nozth = _run(ctx, f, mh, ml, drop=("ZTH",))
    for k in G.SWK_OUT:
        np.testing.assert_array_equal(nozth[k], full[k], err_msg=k)


def _shared_optics_fields(dt, ncol=70, lm=9):
    """70 columns (a full wavefront and a partial one) x 9 layers (getvistau's run of 8 layers and a tail of one; an odd tail of this
    kernel's two-layer walk), super-layers 1-2 / 3-5 / 6-9: condensate over five decades, covers and radii with every special case"""
    rng = np.random.default_rng(41)
    f = {"PLE": np.linspace(1000.0, 100000.0, lm + 1)[:, None] * rng.uniform(0.97, 1.03, ncol), "ZTH": rng.uniform(0.05, 1.0, ncol),
         "T": rng.uniform(210.0, 290.0, (lm, ncol)), "FCLD": rng.uniform(0.0, 1.0, (lm, ncol))}
    f["FCLD"][rng.uniform(0, 1, (lm, ncol)) < 0.15] = 0.005
    f["FCLD"][rng.uniform(0, 1, (lm, ncol)) < 0.10] = 0.0
    for q in ("QI", "QL", "QR", "QS"):
        f[q] = 10.0 ** rng.uniform(-8.0, -3.0, (lm, ncol))
    for r, (lo, hi) in (("RI", (15e-6, 60e-6)), ("RL", (6e-6, 20e-6)), ("RR", (50e-6, 200e-6)), ("RS", (40e-6, 200e-6))):
        f[r] = rng.uniform(lo, hi, (lm, ncol))
        f[r][rng.uniform(0, 1, (lm, ncol)) < 0.08] = 0.0
        f[r][rng.uniform(0, 1, (lm, ncol)) < 0.04] = -1e-6
    return {k: np.ascontiguousarray(v, dtype=dt) for k, v in f.items()}, 3, 6


@pytest.mark.gpu
@pytest.mark.parametrize("rk", [4, 8])
def test_species_thicknesses_are_getvistaus_taudiff_bit_for_bit(gpu_ctx, rk):
    """TAUCLI / TAUCLW / TAUCLR / TAUCLS = geosrad_getvistau_dev's taudiff(:,:,1:4) on the same fields, bit for bit: both kernels take
    the species' thicknesses, the table index step and the caif scaling from the same device functions"""
    import torch
    ctx = gpu_ctx[rk]; dt = ctx.dtype
    f, mh, ml = _shared_optics_fields(dt)
    lm, ncol = f["FCLD"].shape
    assert (ncol, lm, mh, ml) == (70, 9, 3, 6)
    tauc = _unscaled(f, dt).astype(dt).sum(axis=0, dtype=dt)
    cloudy = (tauc > dt(0.02)) & (f["FCLD"] > dt(0.01))
    assert (tauc <= dt(0.02)).any() and (tauc > dt(32.)).any() and (f["FCLD"] <= dt(0.01)).any()
    assert all((f[r] <= 0).any() for r in ("RI", "RL", "RS")) and (f["RS"] * dt(1.e6) > dt(112.0)).any()
    assert cloudy[:mh - 1].any() and cloudy[mh - 1:ml - 1].any() and cloudy[ml - 1:].any() and (tauc[cloudy] > dt(32.)).any()
    names = ["TAUCLI", "TAUCLW", "TAUCLR", "TAUCLS"]
    got = _run(ctx, f, mh, ml, names=names)
    a = {"cosz": f["ZTH"], "dp": f["PLE"][1:] - f["PLE"][:-1], "fcld": f["FCLD"],
         "reff": np.stack([f[k] * dt(1.e6) for k in ("RI", "RL", "RR", "RS")]), "hydromets": np.stack([f[k] for k in ("QI", "QL", "QR", "QS")])}
    assert all(v.dtype == dt for v in a.values())
    t = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in a.items()}
    t["taudiff"] = torch.full((4, lm, ncol), -7.0, dtype=t["dp"].dtype, device="cuda")
    try:
        ctx.getvistau_dev(_stream(), ncol, lm, {k: v.data_ptr() for k, v in t.items()}, mh, ml, grav=9.80665)
        ctx.check(_stream())
    finally:
        torch.cuda.synchronize()
    taudiff = t["taudiff"].cpu().numpy()
    assert (taudiff[:, cloudy] > 0).any() and (taudiff[:, ~cloudy] == 0).all()
    for s, k in enumerate(names):
        np.testing.assert_array_equal(got[k].view(np.uint32 if rk == 4 else np.uint64), taudiff[s].view(np.uint32 if rk == 4 else np.uint64), err_msg=k)


@pytest.mark.gpu
@pytest.mark.parametrize("rk", [4, 8])
def test_null_exports_untouched_and_einval_writes_nothing(gpu_ctx, rk):
    from geosradiation_gridcomp_amd import gridcomp as G
    from geosradiation_gridcomp_amd.api import Context, GeosradError
    ctx = gpu_ctx[rk]
    f, mh, ml = _fields(300, start=5100, seed=11)
    f = {k: v.astype(ctx.dtype) for k, v in f.items()}
    some = ["TAUCLW", "CLDHI", "COTDENTT", "TAUTX", "COTMD", "COTNUMLO", "CLDPRS"]
    o = _run(ctx, f, mh, ml, names=some, sentinel=-3.0)
    for k in G.SWK_OUT:
        assert ((o[k] == -3.0).all()) == (k not in some), k
    lm = f["FCLD"].shape[0]
    bad = [dict(mh=1, ml=ml), dict(mh=ml, ml=ml), dict(mh=mh, ml=lm + 1), dict(mh=ml, ml=mh),
           dict(drop=("FCLD",), names=["CLDLO"]), dict(drop=("QS",), names=["TAULO"]), dict(drop=("RI",), names=["TAUCLI"]),
           dict(drop=("PLE",), names=["CLDPRS"]), dict(drop=("T",), names=["CLDTMP"])]
    for b in bad:
        with pytest.raises(GeosradError):
            o = _run(ctx, f, b.get("mh", mh), b.get("ml", ml), names=b.get("names"), drop=b.get("drop", ()), sentinel=-5.0)
    # inputs an export does not need may be NULL: the cloud fractions from FCLD alone
    frac = _run(ctx, f, mh, ml, names=["CLDLO", "FCLD_X", "COTDENHI"], drop=("PLE", "T", "QI", "QL", "QR", "QS", "RI", "RL", "RR", "RS", "ZTH"))
    full = _run(ctx, f, mh, ml)
    for k in ("CLDLO", "FCLD_X", "COTDENHI"):
        np.testing.assert_array_equal(frac[k], full[k], err_msg=k)
    # ncol / lm not positive, tables not set: EINVAL, nothing written
    import torch
    tdt = torch.float32 if rk == 4 else torch.float64
    sent = torch.full((8,), -5.0, dtype=tdt, device="cuda")
    fc = torch.zeros((4, 8), dtype=tdt, device="cuda")
    for ncol, lmx, c in ((0, 4, ctx), (8, 0, ctx)):
        with pytest.raises(GeosradError):
            c.sw_update_clouds_dev(_stream(), ncol, lmx, 2, 3, TAUCRIT, {"FCLD": fc.data_ptr(), "CLDLO": sent.data_ptr()})
    bare = Context(rk, tables=False)
    try:
        with pytest.raises(GeosradError, match="tables not set"):
            bare.sw_update_clouds_dev(_stream(), 8, 4, 2, 3, TAUCRIT, {"FCLD": fc.data_ptr(), "CLDLO": sent.data_ptr()})
    finally:
        bare.close()
    torch.cuda.synchronize()
    assert (sent == -5.0).all().item()


@pytest.mark.gpu
@pytest.mark.parametrize("rk", [4, 8])
def test_einval_leaves_every_buffer_untouched(gpu_ctx, rk):
    import torch
    from geosradiation_gridcomp_amd import gridcomp as G
    from geosradiation_gridcomp_amd.api import GeosradError
    ctx = gpu_ctx[rk]; dt = ctx.dtype
    f, mh, ml = _fields(300, start=5200, seed=12)
    lm, ncol = f["FCLD"].shape
    tdt = torch.float32 if rk == 4 else torch.float64
    t = {k: torch.from_numpy(np.ascontiguousarray(f[k], dtype=dt)).cuda() for k in G.SWK_IN}
    o = {k: torch.full((lm, ncol) if k in G.SWK_OUT_3D else (ncol,), -5.0, dtype=tdt, device="cuda") for k in G.SWK_OUT}
    for mhx, mlx, drop in ((1, ml, None), (mh, lm + 1, None), (mh, ml, "QL"), (mh, ml, "T")):
        ptr = {k: v.data_ptr() for k, v in t.items() if k != drop}
        ptr.update({k: v.data_ptr() for k, v in o.items()})
        with pytest.raises(GeosradError):
            ctx.sw_update_clouds_dev(_stream(), ncol, lm, mhx, mlx, TAUCRIT, ptr)
    torch.cuda.synchronize()
    for k, v in o.items():
        assert (v == -5.0).all().item(), k


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["r8", "r4"])
def test_fortran_caller_equals_c_entry_point(tmp_path, gpu_ctx, kind):
    """swclouds_driver.F90: `call sw_update_clouds` (module geosrad_gridcomp) on device fields gives the C entry point's bits"""
    from geosradiation_gridcomp_amd import gridcomp as G
    fdir = os.path.join(ROOT, "geosradiation_gridcomp_amd", "fortran")
    exe = os.path.join(fdir, "bin", f"swclouds_driver_{kind}")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-s", "-C", fdir])
    f, mh, ml = _fields(333, start=6100, seed=13)
    f32 = {k: np.ascontiguousarray(f[k], dtype=np.float32) for k in G.SWK_IN}
    lm, ncol = f32["FCLD"].shape
    fin, fout = tmp_path / "in.bin", tmp_path / "out.bin"
    with open(fin, "wb") as fh:
        np.array([ncol, lm, mh, ml], dtype=np.int32).tofile(fh)
        np.array([TAUCRIT], dtype=np.float64).tofile(fh)
        for k in G.SWK_IN:
            f32[k].tofile(fh)
    env = dict(os.environ, GEOSRAD_DATA=os.path.join(ROOT, "geosradiation_gridcomp_amd", "data"))
    subprocess.check_call([exe, str(fin), str(fout)], env=env)
    raw = np.fromfile(fout, dtype=np.float64)
    sizes = [lm * ncol if k in G.SWK_OUT_3D else ncol for k in G.SWK_OUT]
    got = dict(zip(G.SWK_OUT, np.split(raw, np.cumsum(sizes)[:-1])))
    ctx = gpu_ctx[4 if kind == "r4" else 8]
    # the Fortran caller passes its own real TAUCRIT and MAPL_GRAV / MAPL_UNDEF of its kind
    want = _run(ctx, f32, mh, ml, taucrit=float(ctx.dtype(TAUCRIT)))
    for k in G.SWK_OUT:
        np.testing.assert_array_equal(got[k], want[k].astype(np.float64).ravel(), err_msg=k)
    assert (got["CLDTMP"] != float(ctx.dtype(1e15))).any()


@pytest.mark.gpu
def test_c360_share_fp32_against_restatement_sample(gpu_ctx, swkref, capsys):
    """one call at a C360 tile's per-GPU share, 97 200 columns x 72 layers, fp32: a seeded sample of 2 000 columns against the
    restatement"""
    ctx = gpu_ctx[4]; dt = np.float32
    base, mh, ml = _fields(4050, start=8100, seed=17)
    rng = np.random.default_rng(23)
    n = 97200
    pick = rng.integers(0, 4050, n)
    scale = rng.uniform(0.2, 3.0, n)
    f = {}
    for k, v in base.items():
        a = v[..., pick] if v.ndim == 2 else v[pick]
        f[k] = np.ascontiguousarray(a * scale if k in ("QI", "QL", "QR", "QS") else a, dtype=dt)
    got = _run(ctx, f, mh, ml)
    s = np.sort(rng.choice(n, 2000, replace=False))
    sub = {k: np.ascontiguousarray(v[..., s]) for k, v in f.items()}
    gs = {k: np.ascontiguousarray(v[..., s]) for k, v in got.items()}
    with capsys.disabled():
        _compare(gs, swkref, sub, mh, ml, dt, report="r4 97200x72 (2000-column sample)")
    _self_consistent(got, f, mh, ml, dt)
