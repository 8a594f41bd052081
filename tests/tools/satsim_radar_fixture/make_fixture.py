"""Regenerates tests/golden/satsim_radar_inputs_72.npz from a checkout of the reference:

    python tests/tools/satsim_radar_fixture/make_fixture.py --ref <GEOSsatsim_GridComp directory> [--work DIR] [--out FILE]

Compiles, unmodified and in place (flang -c -O1 -ffp-contract=off), the reference's llnl/prec_scops.f in r4 and r8 (-fdefault-real-8) with
driver.f90, and quickbeam/mrgrnk.f90, array_lib.f90, math_lib.f90 and gases.f90 in one plain build with driver_gases.f90: mrgrnk.f90 does not
compile under -fdefault-real-8 (the real and the double procedure of its generic collide), and quickbeam is real*8 throughout, so one build
serves both kinds - the real-kind unit conversions of cosp_radar.F90:136-139 are done here in numpy (radar_inputs_util.radar_gases states
them), for float32 and float64 inputs and for a spaceborne and a surface radar.

The batch is that of tests/golden/satsim_isccp_72.npz (96 x 72 x 30; pfull, at and the overlap-3 mask are read from that file, not stored
again) with make_hydro()'s zfull as zlev, radar_inputs_util.make_radar_inputs()'s precipitation and humidity, and five levels of the mask
replaced (radar_inputs_util.make_mask_edit; stored as mask_edit): the batch has no cloud above level 58, and prec_scops' first-level
branches need one.

Asserts and stores the batch's coverage ("change the batch, not the bound"; radar_inputs_util.COVERAGE): every possibility of prec_scops
of both kinds at the first level (ONE, THREE, Four, Five; TWO needs a level above) and ONE to Five below it, cells with both kinds, THREE
at ilev = nlev - 1 and its skip at ilev = nlev, precipitation in clear cells, both branches of path_integral.  Asserts that prec_frac is
the same from the r4 and the r8 build and equals the numpy restatement's, and stores it as bytes with g_vol and g_to_vol of the four runs
and what the float64 restatement differs from them (restate64rel_*).  Nothing of the reference is copied into the repository."""
import argparse
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(HERE))))
from tests import satsim_util as U  # noqa: E402
from tests import satsim_misr_modis_util as M  # noqa: E402
from tests import radar_inputs_util as RU  # noqa: E402

NP, NL, NC = 96, 72, 30
FLAGS = ["-O1", "-ffp-contract=off"]
QUICKBEAM = ("quickbeam/mrgrnk.f90", "quickbeam/array_lib.f90", "quickbeam/math_lib.f90", "quickbeam/gases.f90")


def compile_in_place(ref, d, sources, driver, fc, flags):
    os.makedirs(d, exist_ok=True)
    objs = []
    for f in sources:
        objs.append(os.path.join(d, os.path.splitext(os.path.basename(f))[0] + ".o"))
        subprocess.check_call([fc, "-c", *flags, "-module-dir", d, "-I" + d, os.path.join(ref, f), "-o", objs[-1]])
    subprocess.check_call([fc, *flags, "-I" + d, "-module-dir", d, os.path.join(HERE, driver), *objs, "-o", os.path.join(d, "driver")])
    return d


def run_prec_scops(d, dt, ls, cv, mask):
    with open(os.path.join(d, "in.bin"), "wb") as f:
        np.array([NP, NL, NC], np.int32).tofile(f)
        for a in (ls, cv, mask):
            np.ascontiguousarray(a, dt).tofile(f)
    t0 = time.perf_counter()
    subprocess.check_call([os.path.join(d, "driver")], cwd=d)
    dt_s = time.perf_counter() - t0
    out = np.fromfile(os.path.join(d, "out.bin"), dt).reshape(NL, NC, NP)
    assert np.isin(out, (0, 1, 2, 3)).all()
    return out.astype(np.uint8), dt_s


def run_gases(d, freq, p_mb, t_c, rh, hgt):
    """the four matrices (ngate, nprof) float64, the radar's first gate first"""
    with open(os.path.join(d, "in.bin"), "wb") as f:
        np.array(p_mb.shape[::-1], np.int32).tofile(f)
        np.array([freq], np.float64).tofile(f)
        for a in (p_mb, t_c, rh, hgt):
            np.ascontiguousarray(a, np.float64).tofile(f)
    t0 = time.perf_counter()
    subprocess.check_call([os.path.join(d, "driver")], cwd=d)
    dt_s = time.perf_counter() - t0
    o = np.fromfile(os.path.join(d, "out.bin"), np.float64).reshape((2,) + p_mb.shape)
    return o[0], o[1], dt_s


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", required=True, help="the reference's GEOSsatsim_GridComp directory")
    ap.add_argument("--work", default=None)
    ap.add_argument("--out", default=RU.FIXTURE)
    ap.add_argument("--fc", default="/opt/rocm/lib/llvm/bin/flang")
    a = ap.parse_args()
    work = a.work or tempfile.mkdtemp(prefix="satsim_radar_fixture_")
    isccp = np.load(U.FIXTURE)
    b0 = {k[3:]: isccp[k] for k in isccp.files if k.startswith("in_") and k != "in_emsfc_lw"}
    assert isccp["mask_ov3"].shape == (NL, NC, NP)
    edit = RU.make_mask_edit(isccp["mask_ov3"])
    mask = RU.fixture_mask(isccp["mask_ov3"], edit)
    assert (mask == 2).any(), "the mask holds no convective cell"
    hy = M.make_hydro(b0)
    x = RU.make_radar_inputs(b0, hy["zfull"])
    fix = {f"in_{k}": v for k, v in x.items()}
    fix["mask_edit"] = edit
    fix["freq"] = np.float64(RU.FREQ)

    # ---- prec_scops: the reference's r4 and r8 builds, on the rates cosp.F90:404-408 forms -------------------------------------
    mr = [hy["ql"], hy["qi"], x["mr_lsrain"], x["mr_lssnow"], hy["qlc"], hy["qic"], x["mr_cvrain"], x["mr_cvsnow"], x["mr_lsgrpl"]]
    pf = {}
    for kind, dt in (("r4", np.float32), ("r8", np.float64)):
        d = compile_in_place(a.ref, os.path.join(work, kind), ("llnl/prec_scops.f",), "driver.f90", a.fc, FLAGS + (["-fdefault-real-8"] if kind == "r8" else []))
        m = [np.asarray(q, dt) for q in mr]
        ls, cv = (m[2] + m[3]) + m[8], m[6] + m[7]
        pf[kind], secs = run_prec_scops(d, dt, ls, cv, mask)
        print(f"prec_scops {kind}: the reference's driver ran {secs * 1e3:.1f} ms for {NP} points (read and write included)")
        mine, poss_ls, poss_cv = RU.prec_scops(ls, cv, mask, dt, detail=True)
        assert np.array_equal(mine, pf[kind]), (kind, "the restatement's prec_frac is not the reference's", int((mine != pf[kind]).sum()))
    assert np.array_equal(pf["r4"], pf["r8"]), "prec_frac differs between the r4 and the r8 build: change the batch"
    fix["prec_frac"] = pf["r4"]
    cov = RU.coverage(pf["r4"], poss_ls, poss_cv, mask)
    print("coverage:", cov)
    assert all(cov[k] > 0 for k in RU.COVERAGE), ("change the batch, not the bound", {k: v for k, v in cov.items() if v <= 0})
    for k in RU.COVERAGE:
        fix[f"count_{k}"] = np.int64(cov[k])
    sg = RU.sghydro(mask, mr, np.float32)
    assert np.array_equal(sg["prec_frac"], pf["r4"])
    dropped = int(((sg["prec_ls"] > 0) & (sg["frac_ls"] == 0) & (np.asarray(mr[2]) > 0)).sum())
    print(f"sghydro: {dropped} (level, point) whose rain no sub-column carries (precipitation under a clear mask)")
    assert dropped > 0, "change the batch, not the bound"
    fix["count_rain_dropped"] = np.int64(dropped)

    # ---- gases and the path integral: one plain build ----------------------------------------------------------------------------
    d = compile_in_place(a.ref, os.path.join(work, "quickbeam"), QUICKBEAM, "driver_gases.f90", a.fc, FLAGS)
    worst = {"g_vol": 0.0, "g_to_vol": 0.0}
    for kind, dt in (("r4", np.float32), ("r8", np.float64)):
        R = np.dtype(dt).type
        p_mb = (np.asarray(b0["pfull"], dt) / R(100.0)).astype(np.float64)          # cosp_radar.F90:136-139
        hgt = (np.asarray(x["zlev"], dt) / R(1000.0)).astype(np.float64)
        t_c = (np.asarray(b0["at"], dt) - R(273.15)).astype(np.float64)
        rh = np.asarray(x["rh"], dt).astype(np.float64)
        for sr in (0, 1):
            o = (lambda q: q[::-1]) if sr else (lambda q: q)                       # order_data: the radar's first gate first
            g_vol, g_to_vol, secs = run_gases(d, RU.FREQ, o(p_mb), o(t_c), o(rh), o(hgt))
            g_vol, g_to_vol = o(g_vol), o(g_to_vol)
            print(f"gases {kind} surface_radar={sr}: the reference's driver ran {secs * 1e3:.1f} ms for {NP} points (read and write included)")
            assert np.isfinite(g_vol).all() and (g_vol > 0).all() and np.isfinite(g_to_vol).all()
            first = NL - 1 if sr else 0
            assert (g_to_vol[first] == 0).all() and (np.delete(g_to_vol, first, axis=0) != 0).all()          # path_integral's empty first gate
            mine = RU.radar_gases(b0["pfull"], b0["at"], x["rh"], x["zlev"], RU.FREQ, sr, dt)
            for n, ref, got in (("g_vol", g_vol, mine[0]), ("g_to_vol", g_to_vol, mine[1])):
                rel = float((np.abs(got - ref) / np.maximum(np.abs(ref), 1e-300)).max())
                print(f"  restatement {n}: max rel |restatement - reference| = {rel:.3e}")
                worst[n] = max(worst[n], rel)
                if n == "g_vol" and sr:          # a volume's own attenuation does not depend on where the radar is: stored once
                    assert np.array_equal(ref, fix[f"{kind}_g_vol"])
                else:
                    fix[f"{kind}_{n}" + ("" if n == "g_vol" else f"_sr{sr}")] = ref
    for n in worst:
        fix[f"restate64rel_{n}"] = np.float64(worst[n])
    np.savez_compressed(a.out, **fix)
    print("wrote", a.out, os.path.getsize(a.out), "bytes,", len(fix), "arrays")


if __name__ == "__main__":
    main()
