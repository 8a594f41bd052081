"""Cost of the radar simulator's front end at 97 200 points x 72 levels x 30 sub-columns (a C360 tile's share, the GEOS default of
SATSIM_NCOLUMNS), in both real kinds: geosrad_prec_scops_dev (k_prec_columns + k_prec_scops), geosrad_cosp_sghydro_dev without and with the
expanded array (the same two + k_sghydro; + k_sghydro_expand), geosrad_radar_gases_dev with g_vol alone (k_radar_gases) and with g_to_vol
(+ k_radar_gas_parab + k_radar_gas_path) - REPS calls of each between two device events after a warm-up, median of ROUNDS rounds; a kernel
that has no entry point of its own is the difference of two rows.  The inputs are the batch of tests/golden/satsim_radar_inputs_72.npz, its
96 points drawn 97 200 times from a seed.  The expanded array (7.5 GB in fp32) is timed at a tenth of the points.
Run from the repository root: python profiles/tools/satsim_radar_inputs_cost.py"""
import sys
import numpy as np
import torch
sys.path.insert(0, ".")
from geosradiation_gridcomp_amd.api import Context
from tests import radar_inputs_util as RU

N, LM, NCOL, REPS, ROUNDS = 97_200, 72, 30, 10, 5
b = RU.load_batch()
pick = np.random.default_rng(23).integers(0, b["mask"].shape[-1], N)
st = torch.cuda.current_stream().cuda_stream


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
    tdt = torch.float32 if rk == 4 else torch.float64
    dev = lambda a, d=dt: torch.from_numpy(np.ascontiguousarray(np.asarray(a)[..., pick], dtype=d)).cuda()
    mask = dev(b["mask"], np.uint8)
    mr = {"mr_" + c: dev(a) for c, a in zip(RU.CLASSES, b["mr"])}
    ls, cv = RU.rates(b["mr"], dt)
    fld = dict(ls_p_rate=dev(ls), cv_p_rate=dev(cv), p=dev(b["p"]), t=dev(b["t"]), rh=dev(b["rh"]), zlev=dev(b["zlev"]))
    prec = torch.empty((LM, NCOL, N), dtype=torch.uint8, device="cuda")
    pl = {k: torch.empty((LM, N), dtype=tdt, device="cuda") for k in ("frac_ls", "frac_cv", "prec_ls", "prec_cv")}
    mr_sub = torch.empty((9, LM, N), dtype=tdt, device="cuda")
    g = {k: torch.empty((LM, N), dtype=torch.float64, device="cuda") for k in ("g_vol", "g_to_vol")}
    n10 = N // 10
    sg10 = torch.empty((9, LM, NCOL, n10), dtype=tdt, device="cuda")
    mask10 = mask[..., :n10].contiguous()
    mr10 = {k: v[..., :n10].contiguous() for k, v in mr.items()}
    P = lambda d: {k: v.data_ptr() for k, v in d.items()}
    pp = dict(P({k: fld[k] for k in ("ls_p_rate", "cv_p_rate")}), frac_out_u8=mask.data_ptr(), prec_frac_u8=prec.data_ptr())
    sp = dict({**P(mr), **P(pl)}, frac_out_u8=mask.data_ptr(), prec_frac_u8=prec.data_ptr(), mr_sub=mr_sub.data_ptr())
    sp10 = dict(P(mr10), frac_out_u8=mask10.data_ptr(), mr_hydro_sg=sg10.data_ptr())
    sp10b = dict(P(mr10), frac_out_u8=mask10.data_ptr(), mr_sub=mr_sub.data_ptr())
    gp = P({k: fld[k] for k in ("p", "t", "rh", "zlev")})
    rows = [
        ("geosrad_prec_scops_dev: k_prec_columns + k_prec_scops", lambda: ctx.prec_scops_dev(st, N, LM, NCOL, pp)),
        ("geosrad_cosp_sghydro_dev: the same + k_sghydro", lambda: ctx.cosp_sghydro_dev(st, N, LM, NCOL, sp)),
        (f"geosrad_cosp_sghydro_dev at {n10} points, mr_sub", lambda: ctx.cosp_sghydro_dev(st, n10, LM, NCOL, sp10b)),
        (f"geosrad_cosp_sghydro_dev at {n10} points, mr_hydro_sg: + k_sghydro_expand", lambda: ctx.cosp_sghydro_dev(st, n10, LM, NCOL, sp10)),
        ("geosrad_radar_gases_dev, g_vol: k_radar_gases", lambda: ctx.radar_gases_dev(st, N, LM, dict(gp, g_vol=g["g_vol"].data_ptr()), RU.FREQ, 0)),
        ("geosrad_radar_gases_dev, g_vol and g_to_vol: + k_radar_gas_parab + k_radar_gas_path", lambda: ctx.radar_gases_dev(st, N, LM, dict(gp, **P(g)), RU.FREQ, 0)),
        ("the same for a surface radar", lambda: ctx.radar_gases_dev(st, N, LM, dict(gp, **P(g)), RU.FREQ, 1)),
    ]
    print(f"real_kind {rk}: {N} x {LM} x {NCOL}, {REPS} calls a round, median of {ROUNDS} (min, max)", flush=True)
    for name, fn in rows:
        med, lo, hi = timed(fn)
        print(f"  {name}: {med:.3f} ms ({lo:.3f}, {hi:.3f})", flush=True)
    ctx.check(st)
    print("  cells with precipitation:", int((prec > 0).sum()), "of", prec.numel(), "; workspace bytes:", ctx.workspace_bytes(), flush=True)
    ctx.close()
