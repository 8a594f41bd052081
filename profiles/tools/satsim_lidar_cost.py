"""Cost of the satellite simulator's lidar path at 97 200 points x 72 levels x 30 sub-columns (a C360 tile's share, the GEOS default of
SATSIM_NCOLUMNS), in both real kinds: geosrad_cosp_lidar_dev (call COSP with ISCCP, MISR, MODIS and the lidar on) beside geosrad_cosp_dev on
the same inputs in the same run, and geosrad_lidar_dev (k_lidar_point + k_lidar_box + k_lidar_stats) alone on the solver-level arrays of the
same call - REPS calls of each between two device events after a warm-up, median of ROUNDS rounds, beside the streaming floor bytes /
6.29 TB/s (the figure of profiles/gettau.md).  With `trace` as the argument nothing is timed: three calls of geosrad_lidar_dev per kind for
a rocprofv3 --kernel-trace --stats run of its own, which gives the three kernels one by one.  The inputs follow the recipes of
tests/satsim_util.make_batch and tests/satsim_misr_modis_util.make_hydro, regenerated here from a seed (nothing is read from a file).
Run from the repository root: python profiles/tools/satsim_lidar_cost.py [trace]"""
import sys
import numpy as np
import torch
sys.path.insert(0, ".")
from geosradiation_gridcomp_amd.api import Context
from tests import satsim_util as U
from tests import satsim_misr_modis_util as M

N, LM, NCOL, REPS, ROUNDS, BASE = 97_200, 72, 30, 10, 5, 1200
HBM = 6.29e12
trace_only = len(sys.argv) > 1 and sys.argv[1] == "trace"
b = U.make_batch(BASE, LM, seed=11)
hy = M.make_hydro(b)
f = U.model_fields(b)
pick = np.random.default_rng(23).integers(0, BASE, N)
st = torch.cuda.current_stream().cuda_stream
COSP_OUT = list(Context.ICARUS_OUT) + ["SGFCLD"] + list(Context.MISR_OUT) + ["modis_mean", "modis_hist"]
LIDAR_OUT = ["clcalipso", "cldlayer", "cfad_sr", "parasolrefl", "lidarpmol"]


def timed(fn):
    fn(); torch.cuda.synchronize()
    ms = []
    for _ in range(ROUNDS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(REPS):
            fn()
        e1.record(); torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1) / REPS)
    return float(np.median(ms)), float(np.min(ms)), float(np.max(ms))


for rk in (4, 8):
    ctx = Context(rk, tables=False)
    dt = ctx.dtype
    E = np.dtype(dt).itemsize
    dev = lambda a, d=dt: torch.from_numpy(np.ascontiguousarray(a[..., pick], dtype=d)).cuda()
    fld = {k: dev(f[k]) for k in ("T", "QV", "FCLD", "CCA", "PLE", "PLO", "DTAU_S", "EMISS", "DTAU_C", "DEM_C", "TS")}
    zle = np.concatenate([(hy["zfull"][0] + 900.)[None, :], 0.5 * (hy["zfull"][:-1] + hy["zfull"][1:]), np.zeros((1, BASE))])
    fld.update(ZLE=dev(zle), QLTOT=dev(hy["ql"]), QITOT=dev(hy["qi"]), RDFL=dev(hy["rl"]), RDFI=dev(hy["ri"]))
    fld["FROCEAN"] = torch.from_numpy((np.arange(N) % 3 != 1).astype(dt)).cuda()
    fld["sunlit"] = dev(f["sunlit"], np.int32)
    fld["seed"] = torch.from_numpy(np.random.default_rng(5).integers(1, 100002, N).astype(np.int32)).cuda()
    tdt = fld["TS"].dtype
    shapes = {"fq_isccp": (7, 7, N), "boxtau": (NCOL, N), "boxptop": (NCOL, N), "SGFCLD": (LM, N), "fq_MISR_TAU_v_CTH": (16, 7, N),
              "dist_model_layertops": (16, N), "modis_mean": (17, N), "modis_hist": (7, 7, N), "clcalipso": (LM, N), "cldlayer": (4, N),
              "cfad_sr": (LM, 15, N), "parasolrefl": (5, N), "lidarpmol": (LM, N)}
    out = {k: torch.empty(shapes.get(k, (N,)), dtype=tdt, device="cuda") for k in COSP_OUT + LIDAR_OUT}
    ptr = {k: v.data_ptr() for k, v in {**fld, **out}.items()}
    cosp_ptr = {k: v for k, v in ptr.items() if k not in LIDAR_OUT + ["FROCEAN"]}
    # the solver-level arrays of the lidar's share of the call, prepared once
    mask = torch.empty((LM, NCOL, N), dtype=torch.uint8, device="cuda")
    seed2 = fld["seed"].clone()
    ctx.scops_dev(st, N, LM, NCOL, {"seed": seed2.data_ptr(), "cc": fld["FCLD"].data_ptr(), "conv": fld["CCA"].data_ptr(),
                                    "frac_out_u8": mask.data_ptr()}, 3)
    presf = torch.cat([torch.zeros((1, N), dtype=tdt, device="cuda"), fld["PLE"][:-1]]).contiguous()
    land = (fld["FROCEAN"] < 0.5).to(tdt)
    lp = {"p": fld["PLO"].data_ptr(), "t": fld["T"].data_ptr(), "presf": presf.data_ptr(), "pplay": fld["PLE"].data_ptr(), "frac_out_u8": mask.data_ptr(),
          "mr_lsliq": fld["QLTOT"].data_ptr(), "mr_lsice": fld["QITOT"].data_ptr(), "reff_lsliq": fld["RDFL"].data_ptr(), "reff_lsice": fld["RDFI"].data_ptr(),
          "land": land.data_ptr(), "lidarcld": out["clcalipso"].data_ptr(), "cldlayer": out["cldlayer"].data_ptr(), "cfad_sr": out["cfad_sr"].data_ptr(),
          "parasolrefl": out["parasolrefl"].data_ptr(), "pmol": out["lidarpmol"].data_ptr()}

    def lidar():
        ctx.lidar_dev(st, N, LM, NCOL, 0, lp)

    if trace_only:
        for _ in range(3):
            lidar()
        torch.cuda.synchronize(); ctx.check(st); ctx.close()
        continue
    pl, cells, boxes = N * LM * E, N * NCOL * LM, N * NCOL
    # k_lidar_point: p, t, presf, four radii in, the mask once, eleven planes and pmol out, three of them read back; k_lidar_box: the mask, the
    # bin plane out, eight planes and four contents and radii and pplay in, the category byte and two depths out; k_lidar_stats: the bin
    # plane and pmol in, lidarcld and 15 cfad planes out, the category byte and the two depths in
    byts = (8 * pl + cells + 12 * pl + 2 * pl) + (2 * cells + 17 * pl + boxes * (1 + 2 * E)) + (cells + pl + 16 * pl + boxes * (1 + 2 * E) + 9 * N * E)
    rows = [
        ("geosrad_cosp_dev (ISCCP + MISR + MODIS)", lambda: ctx.cosp_dev(st, N, LM, NCOL, cosp_ptr), None),
        ("geosrad_cosp_lidar_dev (the same + the lidar)", lambda: ctx.cosp_lidar_dev(st, N, LM, NCOL, ptr), None),
        ("geosrad_lidar_dev: k_lidar_point + _box + _stats", lidar, byts),
    ]
    print(f"real_kind {rk}: {N} x {LM} x {NCOL}, {REPS} calls a round, median of {ROUNDS} (min, max)", flush=True)
    for name, fn, by in rows:
        med, lo, hi = timed(fn)
        floor = "" if by is None else f"; {by / 1e6:.0f} MB, floor {by / HBM * 1e3:.3f} ms = {100 * by / HBM * 1e3 / med:.0f} % of the time"
        print(f"  {name}: {med:.3f} ms ({lo:.3f}, {hi:.3f}){floor}", flush=True)
    ctx.check(st)
    cld = out["clcalipso"]
    print("  cloudy cells of the mask:", int((mask > 0).sum()), "of", cells, "; (point, level) with lidar cloud:", int(((cld > 0) & (cld > -1e29)).sum()),
          "; undefined:", int((cld < -1e29).sum()), "; workspace bytes:", ctx.workspace_bytes(), flush=True)
    ctx.close()
