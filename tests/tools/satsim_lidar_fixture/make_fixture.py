"""Regenerates tests/golden/satsim_lidar_72.npz from a checkout of the reference:

    python tests/tools/satsim_lidar_fixture/make_fixture.py --ref <GEOSsatsim_GridComp directory> [--work DIR] [--out FILE]

Compiles the reference's cosp_constants.F90, llnl/llnl_stats.F90, actsim/lmd_ipsl_stats.F90 and actsim/lidar_simulator.F90 unmodified, in
place, in r4 and r8 (flang -c -O1 -ffp-contract=off; r8 adds -fdefault-real-8) with driver.f90 beside them in a work directory - the four
build with no other module of the reference - and runs both builds, for ice_type 0 and 1, on the batch of tests/golden/satsim_isccp_72.npz
(its inputs and its overlap-3 mask are read from that file, not stored again) with satsim_misr_modis_util.make_hydro()'s contents and
radii, thickened on every fifth point (lidar_util.thicken), and lidar_util.make_lidar_inputs() (thin layers on every sixth point): lidar_simulator once per sub-column on the
in-cloud arrays numpy prepares by COSP's rules (lidar_util.subcolumns), diag_lidar on the collected arrays.  The reference counts its levels
from the surface: the arrays are flipped on the way in and out, nothing else.

Asserts and prints the batch's coverage ("change the batch, not the bound") and the reference's own agreement - between the r4 and the r8
build the bin, cloudy and usable decisions differ in at most 0.1 % of the cells, no r8 ratio lies within 1e-9 relative of a bin edge, and
the numpy restatement gives the r4 build's discrete results exactly - and stores the lidar's own inputs, the statistics (cfad_sr as counts)
and pmol of both builds in full, beta_tot, tau_tot and refl of both builds for a sample of points, the r4-against-r8 spread of every
continuous output (spread_*) and what the float64 restatement differs from the r8 build (restate64rel_*).  Nothing of the reference is
copied into the repository."""
import argparse
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(HERE))))
from tests import satsim_util as U  # noqa: E402
from tests import satsim_misr_modis_util as M  # noqa: E402
from tests import lidar_util as LU  # noqa: E402

NP, NL, NC = 96, 72, 30
SAMPLE = np.array([1, 2, 7, 22, 40, 77])          # the points whose per-sub-column outputs are stored
SOURCES = ("cosp_constants.F90", "llnl/llnl_stats.F90", "actsim/lmd_ipsl_stats.F90", "actsim/lidar_simulator.F90")


def build(ref, work, kind, fc):
    d = os.path.join(work, kind)
    os.makedirs(d, exist_ok=True)
    flags = ["-O1", "-ffp-contract=off"] + (["-fdefault-real-8"] if kind == "r8" else [])
    objs = []
    for f in SOURCES:
        objs.append(os.path.join(d, os.path.basename(f)[:-4] + ".o"))
        subprocess.check_call([fc, "-c", *flags, "-I" + ref, "-module-dir", d, os.path.join(ref, f), "-o", objs[-1]])
    subprocess.check_call([fc, *flags, "-I" + d, "-module-dir", d, os.path.join(HERE, "driver.f90"), *objs, "-o", os.path.join(d, "driver")])
    return d


def run(d, kind, ice_type, b):
    """one run of the driver: the arrays go in and come out surface first, as the reference holds them"""
    dt = np.float32 if kind == "r4" else np.float64
    cells = LU.subcolumns(b["mask"], b["mr_lsliq"], b["mr_lsice"], b["mr_cvliq"], b["mr_cvice"], dt)
    flip = lambda a: np.ascontiguousarray(np.asarray(a, dt)[::-1])
    with open(os.path.join(d, "in.bin"), "wb") as f:
        np.array([NP, NL, NC, ice_type], np.int32).tofile(f)
        flip(b["p"]).tofile(f); flip(b["t"]).tofile(f); flip(b["presf"]).tofile(f)
        for c in cells:
            flip(c).tofile(f)
        for n in ("reff_lsliq", "reff_lsice", "reff_cvliq", "reff_cvice"):
            flip(b[n]).tofile(f)
        flip(b["mask"]).tofile(f); np.asarray(b["land"], dt).tofile(f); flip(b["pplay"]).tofile(f)
    subprocess.check_call([os.path.join(d, "driver")], cwd=d)
    raw = open(os.path.join(d, "out.bin"), "rb")
    rd = lambda *shape: np.fromfile(raw, dt, int(np.prod(shape))).reshape(shape)
    o = dict(pmol=rd(NL, NP)[::-1], beta_tot=rd(NL, NC, NP)[::-1], tau_tot=rd(NL, NC, NP)[::-1], refl=rd(5, NC, NP), lidarcld=rd(NL, NP)[::-1],
             cldlayer=rd(4, NP), cfad_sr=rd(NL, 15, NP)[::-1], parasolrefl=rd(5, NP))
    sr = rd(15)
    assert raw.read() == b""
    assert np.array_equal(sr, np.array(LU.srbval(dt), dt)), "the restatement's bin edges are not the reference's"
    # cosp_stats.F90:137-140
    for n in LU.STATS:
        o[n] = np.where(o[n] == dt(LU.LIDAR_UNDEF), dt(LU.R_UNDEF), o[n]).astype(dt)
    return {k: np.ascontiguousarray(v) for k, v in o.items()}


def decisions(o, dt):
    """the bin, cloudy and usable decision of every cell from a build's own pnorm and pmol"""
    code, x = LU.bin_codes(o["beta_tot"], o["pmol"], dt)
    return code, x


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", required=True, help="the reference's GEOSsatsim_GridComp directory")
    ap.add_argument("--work", default=None)
    ap.add_argument("--out", default=LU.FIXTURE)
    ap.add_argument("--fc", default="/opt/rocm/lib/llvm/bin/flang")
    a = ap.parse_args()
    work = a.work or tempfile.mkdtemp(prefix="satsim_lidar_fixture_")
    isccp = np.load(U.FIXTURE)
    b0 = {k[3:]: isccp[k] for k in isccp.files if k.startswith("in_") and k != "in_emsfc_lw"}
    mask = isccp["mask_ov3"]
    assert mask.shape == (NL, NC, NP)
    hy = LU.thicken(M.make_hydro(b0), b0)
    extra = LU.make_lidar_inputs(b0)
    b = dict(p=extra["p"], t=b0["at"], presf=extra["presf"], pplay=extra["pplay"], land=extra["land"], mask=mask, mr_lsliq=hy["ql"], mr_lsice=hy["qi"],
             mr_cvliq=hy["qlc"], mr_cvice=hy["qic"], reff_lsliq=hy["rl"], reff_lsice=hy["ri"], reff_cvliq=hy["rlc"], reff_cvice=hy["ric"])
    fix = {f"in_{k}": b[k] for k in ("p", "presf", "pplay", "mr_lsliq", "mr_lsice", "mr_cvliq", "mr_cvice", "land")}
    fix["sample"] = SAMPLE
    dirs = {k: build(a.ref, work, k, a.fc) for k in ("r4", "r8")}
    for ice in (0, 1):
        tag = f"_ice{ice}"
        r4, r8 = (run(dirs[k], k, ice, b) for k in ("r4", "r8"))
        c4, _ = decisions(r4, np.float32)
        c8, x8 = decisions(r8, np.float64)
        # coverage
        cnt = LU.cfad_counts(r8["cfad_sr"], NC)
        bins = int((np.where(cnt > 0, cnt, 0).sum(axis=(0, 2)) > 0).sum())
        above, att = int((c8 == LU.ABOVE).sum()), int((c8 == 0).sum())
        dead = int((r8["lidarcld"] == LU.R_UNDEF).sum())
        cat = (r8["cldlayer"][:3] > 0) & (r8["cldlayer"][:3] != LU.R_UNDEF)
        print(f"ice_type {ice}: {bins} of 15 bins populated, {above} cells above the last bin, {att} fully attenuated cells, {dead} (point, level) "
              f"without a usable sub-column, points with low / mid / high cloud {cat.sum(axis=1).tolist()}, "
              f"{int((b['land'] == 1).sum())} land and {int((b['land'] == 0).sum())} ocean points")
        assert bins >= 14 and above > 0 and att > 0 and dead > 0 and cat.any(axis=1).all(), "change the batch, not the bound"
        assert (b["land"] == 1).any() and (b["land"] == 0).any()
        assert (r8["parasolrefl"][:, b["land"] == 1] == LU.R_UNDEF).all() and (r8["parasolrefl"][:, b["land"] == 0] != LU.R_UNDEF).all()
        # the reference's own agreement
        cl = lambda c: (c >= 4) & (c <= LU.ABOVE)
        us = lambda c: (c >= 1) & (c <= LU.ABOVE)
        moved = int(((c4 != c8) | (cl(c4) != cl(c8)) | (us(c4) != us(c8))).sum())
        print(f"  r4 against r8: {moved} of {c8.size} cells with another bin, cloudy or usable decision ({100. * moved / c8.size:.4f} %, cap 0.1 %)")
        assert moved <= 0.001 * c8.size, "change the batch, not the bound"
        edges = np.array(LU.srbval(np.float64))
        near = np.abs(x8[..., None] - edges) <= 1e-9 * edges
        assert not near[c8 != LU.UNDEF_CODE].any(), "an r8 ratio within 1e-9 relative of a bin edge: change the batch, not the bound"
        d4 = np.abs(LU.cfad_counts(r4["cfad_sr"], NC) - cnt)
        print(f"  cfad_sr counts r4 against r8: {int(d4.sum() + 1) // 2} sub-columns in another bin")
        for n in LU.CONTINUOUS:
            ok = (r8[n] != LU.R_UNDEF) & (r4[n] != np.float32(LU.R_UNDEF))
            if n in ("lidarcld", "cldlayer"):      # only where the counts behind the fraction agree; a moved decision is counted above
                ok &= np.abs(r4[n].astype(np.float64) - r8[n]) < 0.5 / NC / NC
            fix[f"spread_{n}{tag}"] = np.float64(np.abs(r4[n].astype(np.float64) - r8[n])[ok].max())
        print("  r4-r8 spread: " + ", ".join(f"{n} {float(fix[f'spread_{n}{tag}']):.2e}" for n in LU.CONTINUOUS))
        # the restatement
        for kind, ref, dt, cref in (("r4", r4, np.float32, c4), ("r8", r8, np.float64, c8)):
            o = LU.lidar(ice, b["p"], b["t"], b["presf"], b["pplay"], mask, b["mr_lsliq"], b["mr_lsice"], b["mr_cvliq"], b["mr_cvice"], b["reff_lsliq"],
                         b["reff_lsice"], b["reff_cvliq"], b["reff_cvice"], b["land"], dt)
            nd = int((o["code"] != cref).sum())
            print(f"  restatement {kind}: {nd} cells with another bin code")
            assert nd == 0, (kind, "the restatement's discrete results are not the reference's")
            assert np.array_equal(LU.cfad_counts(o["cfad_sr"], NC), LU.cfad_counts(ref["cfad_sr"], NC)), (kind, "cfad_sr")
            for n in ("lidarcld", "cldlayer", "cfad_sr"):
                assert np.array_equal(o[n], ref[n]), (kind, n)
            assert np.array_equal(o["parasolrefl"] == dt(LU.R_UNDEF), ref["parasolrefl"] == dt(LU.R_UNDEF)), kind
            for n in ("parasolrefl", "pmol", "beta_tot", "tau_tot", "refl"):
                ok = ref[n] != dt(LU.R_UNDEF)
                d = (np.abs(o[n].astype(np.float64) - ref[n].astype(np.float64)) / np.maximum(np.abs(ref[n].astype(np.float64)), 1e-300))[ok]
                exact = np.array_equal(o[n], ref[n])
                print(f"  restatement {kind} {n}: max rel |restatement - reference| = {d.max():.3e}{' (bit for bit)' if exact else ''}")
                if kind == "r8":
                    fix[f"restate64rel_{n}{tag}"] = np.float64(d.max())
                else:
                    fix[f"restate32exact_{n}{tag}"] = np.bool_(exact)
            fix[f"{kind}_cfad_counts{tag}"] = LU.cfad_counts(ref["cfad_sr"], NC).astype(np.int8)
            for n in ("lidarcld", "cldlayer", "parasolrefl", "pmol"):
                fix[f"{kind}_{n}{tag}"] = ref[n]
            for n in ("beta_tot", "tau_tot", "refl"):
                fix[f"{kind}_{n}{tag}"] = np.ascontiguousarray(ref[n][..., SAMPLE])
            fix[f"{kind}_code{tag}"] = cref
    np.savez_compressed(a.out, **fix)
    print("wrote", a.out, os.path.getsize(a.out), "bytes,", len(fix), "arrays")


if __name__ == "__main__":
    main()
