"""Cost of the MISR simulator at 97 200 points x 72 levels x 30 sub-columns (a C360 tile's share, the GEOS default of SATSIM_NCOLUMNS), in
both real kinds: geosrad_misr_dev (k_misr_box + k_misr_stats) on the overlap-3 mask geosrad_scops_dev leaves - REPS calls between two
device events after a warm-up, median of ROUNDS rounds, beside the mask's bytes over the time.  The inputs are
tests/satsim_util.make_batch and tests/satsim_misr_modis_util.make_hydro at that size, regenerated here from their seeds (nothing is read
from a file).  Run from the repository root: python profiles/tools/satsim_misr_cost.py"""
import sys
import numpy as np
import torch
sys.path.insert(0, ".")
from geosradiation_gridcomp_amd.api import Context
from tests import satsim_util as U
from tests import satsim_misr_modis_util as M

N, LM, NCOL, REPS, ROUNDS = 97_200, 72, 30, 50, 5
b = U.make_batch(N, LM)
b.update(M.make_hydro(b))
st = torch.cuda.current_stream().cuda_stream

for rk in (4, 8):
    ctx = Context(rk, tables=False)
    dev = lambda a, d: torch.from_numpy(np.ascontiguousarray(a, dtype=d)).cuda()
    t = {k: dev(b[k], ctx.dtype) for k in ("zfull", "at", "dtau_s", "dtau_c", "cc", "conv")}
    t["sunlit"], t["seed"] = dev(b["sunlit"], np.int32), dev(b["seed"], np.int32)
    t["frac_out_u8"] = torch.zeros((LM, NCOL, N), dtype=torch.uint8, device="cuda")
    tdt = t["at"].dtype
    t.update({"fq_MISR_TAU_v_CTH": torch.empty((16, 7, N), dtype=tdt, device="cuda"), "dist_model_layertops": torch.empty((16, N), dtype=tdt, device="cuda"),
              "MISR_mean_ztop": torch.empty(N, dtype=tdt, device="cuda"), "MISR_cldarea": torch.empty(N, dtype=tdt, device="cuda")})
    ptr = {k: v.data_ptr() for k, v in t.items()}
    ctx.scops_dev(st, N, LM, NCOL, ptr, 3)
    for _ in range(3):
        ctx.misr_dev(st, N, LM, NCOL, ptr, M.MISSING)
    torch.cuda.synchronize()
    ms = []
    for _ in range(ROUNDS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(REPS):
            ctx.misr_dev(st, N, LM, NCOL, ptr, M.MISSING)
        e1.record(); torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1) / REPS)
    ctx.check(st)
    med, cells = float(np.median(ms)), N * NCOL * LM
    print(f"real_kind {rk}: geosrad_misr_dev at {N} x {LM} x {NCOL}, {REPS} calls a round, median of {ROUNDS} (min, max): {med:.3f} ms "
          f"({min(ms):.3f}, {max(ms):.3f}); mask {cells / 1e6:.0f} MB = {cells / 1e6 / med:.0f} GB/s of mask alone; points with cloud: "
          f"{int((t['MISR_cldarea'] > 0).sum())}; workspace bytes: {ctx.workspace_bytes()}", flush=True)
    ctx.close()
