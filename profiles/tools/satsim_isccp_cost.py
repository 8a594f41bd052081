"""Cost of the satellite simulator's ISCCP path at 97 200 points x 72 levels x 30 sub-columns (a C360 tile's share, the GEOS default of
SATSIM_NCOLUMNS), in both real kinds: geosrad_isccp_dev (SCOPS + SGFCLD + ICARUS, the mask in the context's workspace) and its parts
through the solver-level entry points - geosrad_scops_dev, geosrad_icarus_dev on that mask, geosrad_cosp_seeds_dev - REPS calls of each
between two device events after a warm-up, median of ROUNDS rounds, beside the streaming floor bytes / 6.29 TB/s (the figure of
profiles/gettau.md).  The mask's own cost in HBM is timed as one device copy of it (one read + one write of npoints x ncol x nlev bytes:
what SCOPS writes and ICARUS reads).  With `trace` as the argument nothing is timed: three calls of geosrad_isccp_dev per kind for a
rocprofv3 --kernel-trace --stats run of its own, which gives the kernels one by one.  The inputs follow the recipe of
tests/satsim_util.make_batch, regenerated here from a seed (nothing is read from a file)."""
import sys
import numpy as np
import torch
sys.path.insert(0, ".")
from geosradiation_gridcomp_amd.api import Context
from tests import satsim_util as U

N, LM, NCOL, REPS, ROUNDS, BASE = 97_200, 72, 30, 10, 5, 1200
HBM = 6.29e12
trace_only = len(sys.argv) > 1 and sys.argv[1] == "trace"
f = U.model_fields(U.make_batch(BASE, LM, seed=11))
pick = np.random.default_rng(23).integers(0, BASE, N)
st = torch.cuda.current_stream().cuda_stream
OUT = list(Context.ICARUS_OUT)


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
    fld = {k: torch.from_numpy(np.ascontiguousarray(f[k][..., pick], dtype=dt)).cuda() for k in ("T", "QV", "FCLD", "CCA", "PLE", "PLO", "DTAU_S", "EMISS",
                                                                                              "DTAU_C", "DEM_C", "TS")}
    fld["sunlit"] = torch.from_numpy(f["sunlit"][pick].astype(np.int32)).cuda()
    seed0 = torch.from_numpy(np.random.default_rng(5).integers(1, 100002, N).astype(np.int32)).cuda()
    fld["seed"] = seed0.clone()
    tdt = fld["TS"].dtype
    shapes = {"fq_isccp": (7, 7, N), "boxtau": (NCOL, N), "boxptop": (NCOL, N)}
    out = {k: torch.empty(shapes.get(k, (N,)), dtype=tdt, device="cuda") for k in OUT}
    out["SGFCLD"] = torch.empty((LM, N), dtype=tdt, device="cuda")
    ptr = {k: v.data_ptr() for k, v in {**fld, **out}.items()}

    def isccp():
        ctx.isccp_dev(st, N, LM, NCOL, ptr)

    if trace_only:
        for _ in range(3):
            isccp()
        torch.cuda.synchronize(); ctx.check(st); ctx.close()
        continue
    # the solver-level arrays of the same call, prepared once
    sc = torch.tensor(0.999999, dtype=tdt, device="cuda")
    phalf = torch.cat([torch.zeros((1, N), dtype=tdt, device="cuda"), fld["PLE"][:-1]]).contiguous()
    mask = torch.empty((LM, NCOL, N), dtype=torch.uint8, device="cuda")
    mask2 = torch.empty_like(mask)
    cc, conv = sc * fld["FCLD"], sc * fld["CCA"]
    sp = {"seed": fld["seed"].data_ptr(), "cc": fld["FCLD"].data_ptr(), "conv": fld["CCA"].data_ptr(), "frac_out_u8": mask.data_ptr()}      # SCOPS: unscaled
    ip = {"sunlit": fld["sunlit"].data_ptr(), "pfull": fld["PLO"].data_ptr(), "phalf": phalf.data_ptr(), "qv": fld["QV"].data_ptr(), "cc": cc.data_ptr(),
          "conv": conv.data_ptr(), "dtau_s": fld["DTAU_S"].data_ptr(), "dtau_c": fld["DTAU_C"].data_ptr(), "frac_out_u8": mask.data_ptr(),
          "skt": fld["TS"].data_ptr(), "at": fld["T"].data_ptr(), "dem_s": fld["EMISS"].data_ptr(), "dem_c": fld["DEM_C"].data_ptr()}
    ip.update({k: out[k].data_ptr() for k in OUT})
    psfc = {"psfc": fld["PLE"][LM].contiguous(), "seed": torch.empty(N, dtype=torch.int32, device="cuda")}
    pl, cells, boxes = N * LM * E, N * NCOL * LM, N * NCOL
    rows = [
        ("geosrad_isccp_dev (all of the below but the seeds)", isccp, None),
        ("geosrad_scops_dev: k_scops", lambda: ctx.scops_dev(st, N, LM, NCOL, sp, 3), 2 * pl + cells + 8 * N),
        ("geosrad_icarus_dev: k_icarus_point + _box + _stats", lambda: ctx.icarus_dev(st, N, LM, NCOL, ip, 1, 2, 3, 0.999),
         (11 + 2) * pl + (cells + 7 * pl + boxes * (3 * E + 1 + 2 * E)) + (boxes * (3 * E + 1) + 55 * N * E)),
        ("geosrad_cosp_seeds_dev: k_cosp_minmax + k_cosp_seeds", lambda: ctx.cosp_seeds_dev(st, N, {k: v.data_ptr() for k, v in psfc.items()}), 2 * N * E + 4 * N),
        ("the mask once each way (a device copy of it)", lambda: mask2.copy_(mask), 2 * cells),
    ]
    print(f"real_kind {rk}: {N} x {LM} x {NCOL}, {REPS} calls a round, median of {ROUNDS} (min, max)", flush=True)
    for name, fn, byts in rows:
        med, lo, hi = timed(fn)
        floor = "" if byts is None else f"; {byts / 1e6:.0f} MB, floor {byts / HBM * 1e3:.3f} ms = {100 * byts / HBM * 1e3 / med:.0f} % of the time"
        print(f"  {name}: {med:.3f} ms ({lo:.3f}, {hi:.3f}){floor}", flush=True)
    ctx.check(st)
    print("  cloudy cells of the mask:", int((mask > 0).sum()), "of", cells, "; workspace bytes:", ctx.workspace_bytes(), flush=True)
    ctx.close()
