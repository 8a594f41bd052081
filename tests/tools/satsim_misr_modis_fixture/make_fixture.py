"""Regenerates tests/golden/satsim_misr_modis_72.npz from a checkout of the reference:

    python tests/tools/satsim_misr_modis_fixture/make_fixture.py --ref <GEOSsatsim_GridComp directory> [--work DIR] [--out FILE]

Compiles the reference's MISR_simulator.f unmodified, in place, in r4 and r8 (flang -c -O1 -ffp-contract=off -I<ref>; r8 adds
-fdefault-real-8) with driver.f90 beside it in a work directory and runs both builds on the batch of tests/golden/satsim_isccp_72.npz (its
inputs and its overlap-3 mask are read from that file, not stored again) plus satsim_misr_modis_util.make_hydro(), as it is and rolled by
one point (point 1 first); and the reference's modis_simulator.F90 (module chain for its .mod files only) with driver_modis.f90, run on the
per-sub-column arrays numpy prepares from the same batch and the ISCCP fixture's r4 boxtau / boxptop.  Checks that the two builds give
identical histograms, layer tops, phases and retrieval status and that the numpy restatement gives them bit for bit, and stores the nine planes, the reference's outputs in both kinds for both orders, its own r4-against-r8 spread per
continuous output (spread_*) and what the float64 restatement differs from the r8 build (restate64_*, restate64rel_modis_*); for MODIS
the L2 results, the 17 means and the joint histogram of both builds on the sunlit points.  Nothing of the reference is
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

NP, NL, NC = 96, 72, 30
SHAPES = dict(fq_MISR_TAU_v_CTH=(16, 7, NP), dist_model_layertops=(16, NP), MISR_mean_ztop=(NP,), MISR_cldarea=(NP,))


def build(ref, work, kind, fc):
    d = os.path.join(work, kind)
    os.makedirs(d, exist_ok=True)
    flags = ["-O1", "-ffp-contract=off"] + (["-fdefault-real-8"] if kind == "r8" else [])
    subprocess.check_call([fc, "-c", *flags, "-I" + ref, os.path.join(ref, "MISR_simulator.f"), "-o", os.path.join(d, "MISR_simulator.o")])
    subprocess.check_call([fc, *flags, os.path.join(HERE, "driver.f90"), os.path.join(d, "MISR_simulator.o"), "-o", os.path.join(d, "driver")])
    return d


def run(d, kind, b, mask):
    dt = np.float32 if kind == "r4" else np.float64
    with open(os.path.join(d, "in.bin"), "wb") as f:
        np.array([NP, NL, NC], np.int32).tofile(f)
        b["sunlit"].astype(np.int32).tofile(f)
        for n in ("zfull", "at", "dtau_s", "dtau_c"):
            b[n].astype(dt).tofile(f)
        mask.astype(dt).tofile(f); np.array([M.MISSING], dt).tofile(f)
    subprocess.check_call([os.path.join(d, "driver")], cwd=d)
    raw = open(os.path.join(d, "out.bin"), "rb")
    o = {n: np.fromfile(raw, dt, int(np.prod(SHAPES[n]))).reshape(SHAPES[n]) for n in M.MISR_OUT}
    assert raw.read() == b""
    assert not any((v == dt(-7.)).any() for v in o.values()), "an output the routine did not set"
    return o


def build_modis(ref, work, kind, fc):
    """the module chain for its .mod files only, modis_simulator.F90 for its object; the driver links that object alone (cosp_types.o
    would pull the radar in)"""
    d = os.path.join(work, kind)
    os.makedirs(d, exist_ok=True)
    flags = ["-O1", "-ffp-contract=off"] + (["-fdefault-real-8"] if kind == "r8" else [])
    for f in ("cosp_constants.F90", "quickbeam/radar_simulator_types.f90", "cosp_utils.F90", "cosp_types.F90", "modis_simulator.F90"):
        subprocess.check_call([fc, "-c", *flags, "-I" + ref, "-module-dir", d, os.path.join(ref, f), "-o", os.path.join(d, os.path.basename(f)[:-4] + ".o")])
    subprocess.check_call([fc, *flags, "-I" + d, "-module-dir", d, os.path.join(HERE, "driver_modis.f90"), os.path.join(d, "modis_simulator.o"), "-o",
                           os.path.join(d, "driver_modis")])
    return d


def run_modis(d, kind, b, mask, boxtau, boxptop):
    """modis_L2_simulator per sunlit point and modis_L3_simulator on the sunlit points, on the per-sub-column arrays numpy prepares by the
    rules of cosp.F90:414-494 and cosp_modis_simulator.F90:138-181 in the build's kind.  Returns the L2 arrays (ncol, nsunlit), the 17
    means (17, nsunlit) and the histogram (7 pressure, 6 tau, nsunlit)"""
    dt = np.float32 if kind == "r4" else np.float64
    lit = b["sunlit"] > 0
    ns = int(lit.sum())
    cells = M.modis_subcolumns(b["dtau_s"], b["dtau_c"], mask, b["ql"], b["qi"], b["qlc"], b["qic"], b["rl"], b["ri"], b["rlc"], b["ric"], dt)
    with open(os.path.join(d, "in_modis.bin"), "wb") as f:
        np.array([ns, NC, NL], np.int32).tofile(f)
        for a in (b["at"], b["pfull"], b["phalf"]):
            a[:, lit].astype(dt).tofile(f)
        for a in cells:
            a[:, :, lit].astype(dt).tofile(f)
        boxtau[:, lit].astype(dt).tofile(f); boxptop[:, lit].astype(dt).tofile(f)
    subprocess.check_call([os.path.join(d, "driver_modis")], cwd=d)
    raw = open(os.path.join(d, "out_modis.bin"), "rb")
    rd = lambda shape, t=dt: np.fromfile(raw, t, int(np.prod(shape))).reshape(shape)
    o = dict(phase=rd((NC, ns), np.int32), ctp=rd((NC, ns)), tau=rd((NC, ns)), size=rd((NC, ns)), mean=rd((17, ns)), hist=rd((7, 6, ns)))
    assert raw.read() == b""
    return o


def modis_section(a, work, b, mask, isccp, fix):
    boxtau, boxptop = isccp["r4_boxtau_th1_d1"], isccp["r4_boxptop_th1_d1"]          # both kinds read the r4 arrays
    lit = b["sunlit"] > 0
    r4, r8 = (run_modis(build_modis(a.ref, work, k, a.fc), k, b, mask, boxtau, boxptop) for k in ("r4", "r8"))
    undef4, undef8 = np.float32(M.R_UNDEF), np.float64(M.R_UNDEF)
    cloudy = r8["phase"] != 0
    got = r8["size"] > 0
    print(f"MODIS: {int(cloudy.sum())} of {cloudy.size} sub-columns cloudy: liquid {int((r8['phase'] == 1).sum())}, ice {int((r8['phase'] == 2).sum())}, "
          f"undetermined {int((r8['phase'] == 3).sum())}; {int(got.sum())} sizes retrieved, {int((cloudy & ~got).sum())} re_fill; "
          f"{int((cloudy & (r8['ctp'] == boxptop[:, lit].astype(np.float64) * 100.)).sum())} take ISCCP's cloud top; "
          f"{int((r8['hist'].sum(axis=2) > 0).sum())} of 42 histogram cells populated")
    assert np.array_equal(r4["phase"], r8["phase"]) and np.array_equal(r4["size"] > 0, got), "change the batch, not the bound"
    assert np.array_equal(np.rint(r4["hist"].astype(np.float64) * NC), np.rint(r8["hist"] * NC)), "change the batch, not the bound"
    for n in ("ctp", "tau", "size"):
        assert np.array_equal(r4[n] == undef4, r8[n] == undef8), n
    rel = lambda x, y: np.abs(x - y) / np.maximum(np.abs(y), 1e-300)
    ok = cloudy
    fix["spread_modis_ctp"] = np.float64(np.abs(r4["ctp"].astype(np.float64) - r8["ctp"])[ok].max())
    fix["spread_modis_tau"] = np.float64(np.abs(r4["tau"].astype(np.float64) - r8["tau"])[ok].max())
    fix["spread_modis_size"] = np.float64(np.abs(r4["size"].astype(np.float64) - r8["size"])[ok].max())
    fix["spread_modis_mean"] = np.abs(r4["mean"].astype(np.float64) - r8["mean"]).max(axis=1)
    print("  r4-r8 spread: size rel", float(rel(r4["size"].astype(np.float64), r8["size"])[got].max()), "mean ctp", float(fix["spread_modis_mean"][14]), "Pa")
    for kind, ref, dt in (("r4", r4, np.float32), ("r8", r8, np.float64)):
        cells = M.modis_subcolumns(b["dtau_s"], b["dtau_c"], mask, b["ql"], b["qi"], b["qlc"], b["qic"], b["rl"], b["ri"], b["rlc"], b["ric"], dt)
        l2 = M.modis_l2(b["at"], b["pfull"], b["phalf"], *cells, boxptop, dt)
        l2 = tuple(x[:, lit] for x in l2)
        mean, hist = M.modis_l3(*l2, dt)
        assert np.array_equal(l2[0], ref["phase"]), (kind, "phase", int((l2[0] != ref["phase"]).sum()))
        assert np.array_equal(l2[3] > 0, ref["size"] > 0), (kind, "retrieved", int(((l2[3] > 0) != (ref["size"] > 0)).sum()))
        assert np.array_equal(hist, ref["hist"]), (kind, "hist")
        for n, x in zip(("ctp", "tau", "size"), l2[1:]):
            assert np.array_equal(x == dt(M.R_UNDEF), ref[n] == dt(M.R_UNDEF)), (kind, n)
            d = rel(x.astype(np.float64), ref[n].astype(np.float64))
            print(f"  restatement {kind} {n}: max rel |restatement - reference| = {d.max():.3e}")
            if kind == "r8":
                fix["restate64rel_modis_" + n] = np.float64(d.max())
        d = rel(mean.astype(np.float64), ref["mean"].astype(np.float64)).max(axis=1)
        print(f"  restatement {kind} means: max rel per mean = {np.array2string(d, precision=2)}")
        if kind == "r8":
            fix["restate64rel_modis_mean"] = d
        for n in ("phase", "ctp", "tau", "size", "mean", "hist"):
            fix[f"{kind}_modis_{n}"] = ref[n]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", required=True, help="the reference's GEOSsatsim_GridComp directory")
    ap.add_argument("--work", default=None)
    ap.add_argument("--out", default=M.FIXTURE)
    ap.add_argument("--fc", default="/opt/rocm/lib/llvm/bin/flang")
    a = ap.parse_args()
    work = a.work or tempfile.mkdtemp(prefix="satsim_misr_modis_fixture_")
    isccp = np.load(U.FIXTURE)
    b = {k[3:]: isccp[k] for k in isccp.files if k.startswith("in_") and k != "in_emsfc_lw"}
    mask = isccp["mask_ov3"]
    assert mask.shape == (NL, NC, NP)
    hy = M.make_hydro(b)
    b.update(hy)
    fix = {f"in_{k}": v for k, v in hy.items()}
    dirs = {k: build(a.ref, work, k, a.fc) for k in ("r4", "r8")}
    for tag, bb, mm in (("", b, mask), ("_rolled", {k: M.roll1(v) for k, v in b.items()}, M.roll1(mask))):
        r4, r8 = (run(dirs[k], k, bb, mm) for k in ("r4", "r8"))
        # the histogram is a sum of 1 / ncol per sub-column in the build's kind: the two builds are compared as counts
        assert np.array_equal(M.misr_counts(r4["fq_MISR_TAU_v_CTH"], NC), M.misr_counts(r8["fq_MISR_TAU_v_CTH"], NC)), (tag, "change the batch, not the bound")
        assert np.array_equal(r4["fq_MISR_TAU_v_CTH"] == np.float32(M.MISSING), r8["fq_MISR_TAU_v_CTH"] == M.MISSING), tag
        assert np.array_equal(r4["dist_model_layertops"], r8["dist_model_layertops"].astype(np.float32)), (tag, "change the batch, not the bound")
        for n in M.MISR_CONTINUOUS:
            assert np.array_equal(r4[n] == np.float32(M.MISSING), r8[n] == M.MISSING), (n, tag)
            ok = r8[n] != M.MISSING
            fix[f"spread_{n}{tag}"] = np.float64(np.abs(r4[n].astype(np.float64) - r8[n])[ok].max())
        lit = bb["sunlit"] == 1
        cnt = M.misr_counts(r8["fq_MISR_TAU_v_CTH"], NC)
        print(f"batch{tag}: {int((r8['MISR_cldarea'][lit] > 0).sum())} of {int(lit.sum())} sunlit points with cloud, "
              f"{int((cnt.sum(axis=(1, 2)) > 0).sum())} of 16 height bins populated, {int(cnt[0].sum())} sub-columns in the no-height bin, "
              f"MISR_mean_ztop r4-r8 spread {float(fix['spread_MISR_mean_ztop' + tag]):.2e} m, last point "
              f"{'sunlit' if lit[-1] else 'dark'}: MISR_mean_ztop {float(r8['MISR_mean_ztop'][-1]):.6g}")
        for kind, ref, dt in (("r4", r4, np.float32), ("r8", r8, np.float64)):
            o = M.misr(bb["sunlit"], bb["zfull"], bb["at"], bb["dtau_s"], bb["dtau_c"], mm, M.MISSING, dt)
            for n in ("fq_MISR_TAU_v_CTH", "dist_model_layertops"):
                assert np.array_equal(o[n], ref[n]), (kind, n, tag)
            for n in M.MISR_CONTINUOUS:
                assert np.array_equal(o[n] == dt(M.MISSING), ref[n] == dt(M.MISSING)), (kind, n, tag)
                d = np.abs(o[n].astype(np.float64) - ref[n].astype(np.float64))[ref[n] != dt(M.MISSING)]
                if kind == "r8":
                    fix[f"restate64_{n}{tag}"] = np.float64(d.max())
                print(f"  restatement {kind} {n}{tag}: max |restatement - reference| = {d.max():.3e}")
            for n in M.MISR_OUT:
                fix[f"{kind}_{n}{tag}"] = ref[n]
    # what the pattern matcher does to a point depends on whether the point is the call's first: each sunlit point rolled to the front
    first = M.misr(b["sunlit"], b["zfull"], b["at"], b["dtau_s"], b["dtau_c"], mask, M.MISSING, np.float64)["MISR_mean_ztop"]
    changed = 0
    for j in np.flatnonzero(b["sunlit"] == 1):
        r = lambda v: np.ascontiguousarray(np.roll(v, -j, axis=-1))
        z = M.misr(r(b["sunlit"]), r(b["zfull"]), r(b["at"]), r(b["dtau_s"]), r(b["dtau_c"]), r(mask), M.MISSING, np.float64)["MISR_mean_ztop"][0]
        changed += int(j > 0 and z != first[j])
    print(f"the pattern matcher changes MISR_mean_ztop of {changed} sunlit points when that point is first; point 1: "
          f"{float(fix['r8_MISR_mean_ztop'][1]):.2f} m second, {float(fix['r8_MISR_mean_ztop_rolled'][0]):.2f} m first")
    assert fix["r8_MISR_mean_ztop"][1] != fix["r8_MISR_mean_ztop_rolled"][0]
    modis_section(a, work, b, mask, isccp, fix)
    np.savez_compressed(a.out, **fix)
    print("wrote", a.out, os.path.getsize(a.out), "bytes,", len(fix), "arrays")


if __name__ == "__main__":
    main()
