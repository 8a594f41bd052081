"""UPDATE_EXPORT's cloud diagnostics (geosrad_sw_update_clouds_dev) at a C360 tile's per-GPU share, 97 200 columns x 72 layers: fp32 and
fp64, every export and a typical subset (the 2-D exports without TAUCL*), 5 launches each after one warm-up.  Run under
rocprofv3 --kernel-trace --stats; also prints host-clock times of the launches (synchronised) and the bytes each configuration moves."""
import sys, time
import numpy as np
import torch
sys.path.insert(0, ".")
from geosradiation_gridcomp_amd import gridcomp as G
from geosradiation_gridcomp_amd.api import Context
from tests.test_sw_clouds import _fields

n, lm, reps = 97200, 72, 5
base, mh, ml = _fields(4050, lm, start=8100, seed=17)
pick = np.random.default_rng(23).integers(0, 4050, n)
f64 = {k: (v[..., pick] if v.ndim == 2 else v[pick]) for k, v in base.items()}
for rk in (4, 8):
    ctx = Context(rk)
    dt = ctx.dtype
    tdt = torch.float32 if rk == 4 else torch.float64
    t = {k: torch.from_numpy(np.ascontiguousarray(v, dtype=dt)).cuda() for k, v in f64.items()}
    o = {k: torch.empty((lm, n) if k in G.SWK_OUT_3D else (n,), dtype=tdt, device="cuda") for k in G.SWK_OUT}
    st = torch.cuda.current_stream().cuda_stream
    for label, names in (("all", G.SWK_OUT), ("2d", G.SWK_OUT_2D)):
        ptr = {k: v.data_ptr() for k, v in t.items()}
        ptr.update({k: o[k].data_ptr() for k in names})
        ctx.sw_update_clouds_dev(st, n, lm, mh, ml, 0.10, ptr)
        torch.cuda.synchronize()
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter()
            ctx.sw_update_clouds_dev(st, n, lm, mh, ml, 0.10, ptr)
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
        nout3 = sum(k in G.SWK_OUT_3D for k in names)
        # nominal traffic: FCLD, QI..QS, RI..RS (9 LM) + PLE (LM+1) read; FCLD read twice; T read at one layer; the requested exports
        byts = (n * (10 * lm + 1 + lm) + n * (nout3 * lm + len(names) - nout3)) * np.dtype(dt).itemsize
        print(f"r{rk} {label}: min {1e3 * min(ts):.3f} ms host-clock per launch, {byts / 1e9:.3f} GB nominal", flush=True)
    ctx.close()
