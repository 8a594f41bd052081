"""Cost of the aerosol-free LW fluxes at 97 200 columns x 72 layers, fp32, 60 % cloudy columns with aerosols:
(a) what a caller had to do without them: geosrad_lw_driver_rrtmg_dev twice, the second time with the aerosol inputs NULL;
(b) one geosrad_lw_driver_rrtmg_na_dev call; (c) the plain driver once.  The three alternate, REPS times each after a warm-up of all;
times from device events around each call.  (a) and (b) must give the same bits.  geosrad_profile gives the kernel slots of (a) and (b)."""
import sys
import numpy as np
import torch
sys.path.insert(0, ".")
from geosradiation_gridcomp_amd import gridcomp as G
from geosradiation_gridcomp_amd import synth
from geosradiation_gridcomp_amd.api import Context

N, LM, REPS, BASE = 97_200, 72, 10, 4000
inp = synth.make_columns(BASE, LM, start=0, cloudy_frac=0.6, aerosol=True)
f = synth.geos_lw_fields(inp)
pick = np.random.default_rng(23).integers(0, BASE, N)
ctx = Context(4)
dt, tdt = ctx.dtype, torch.float32
ctx.set_inhomogeneity(1)
fld = {k: torch.from_numpy(np.ascontiguousarray(v[..., pick], dtype=dt)).cuda() for k, v in f.items() if isinstance(v, np.ndarray)}
consts = G.lwd_consts()
doy, llm, lmh = int(inp["dyofyr"]), f["LCLDLM"], f["LCLDMH"]
shape = lambda k: (LM + 1, N) if k in G.LWD_OUT_3D else (N,)
mk = lambda names: {k: torch.empty(shape(k), dtype=tdt, device="cuda") for k in names}
out, out2 = mk(G.LWD_OUT[:16]), mk(G.LWD_OUT[:16])
na = {k: torch.empty((LM + 1, N), dtype=tdt, device="cuda") for k in G.LWNA_OUT}
st = torch.cuda.current_stream().cuda_stream
pin = {k: v.data_ptr() for k, v in fld.items()}
ptr = lambda o, aer=True: {**{k: v for k, v in pin.items() if aer or k not in ("TAUA", "SSAA")}, **{k: v.data_ptr() for k, v in o.items()}}


def twice():
    ctx.lw_driver_rrtmg_dev(st, N, LM, 16, ptr(out), consts, 3, 1, doy, llm, lmh)
    ctx.lw_driver_rrtmg_dev(st, N, LM, 0, ptr(out2, aer=False), consts, 3, 1, doy, llm, lmh)


def shared():
    ctx.lw_driver_rrtmg_na_dev(st, N, LM, 16, ptr(out), consts, 3, 1, doy, llm, lmh, {k: v.data_ptr() for k, v in na.items()})


def plain():
    ctx.lw_driver_rrtmg_dev(st, N, LM, 16, ptr(out), consts, 3, 1, doy, llm, lmh)


fns = (twice, shared, plain)
twice(); ctx.check(st)
a = {k: v.clone() for k, v in out.items()}; a2 = {k: v.clone() for k, v in out2.items()}
shared(); ctx.check(st)
pairs = (("FLXAU_INT", "FLXU_INT"), ("FLXAD_INT", "FLXD_INT"), ("FLAU_INT", "FLCU_INT"), ("FLAD_INT", "FLCD_INT"), ("FLXA_INT", "FLX_INT"),
         ("FLA_INT", "FLC_INT"), ("DFDTSNA", "DFDTS"), ("DFDTSCNA", "DFDTSC"))
same = all(torch.equal(out[k], a[k]) for k in out) and all(torch.equal(na[x], a2[y]) for x, y in pairs)
print("outputs of (a) and (b) bitwise equal:", same, flush=True)
plain(); torch.cuda.synchronize()
times = {fn.__name__: [] for fn in fns}
for _ in range(REPS):
    for fn in fns:
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record(); torch.cuda.synchronize()
        times[fn.__name__].append(e0.elapsed_time(e1))
for k, v in times.items():
    v = np.array(v)
    print(f"{k}: median {np.median(v):.3f} ms, min {v.min():.3f}, max {v.max():.3f}, std {v.std():.3f} over {REPS} calls", flush=True)
for fn in (twice, shared):
    ctx.profile(True)
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    pr = {k: v for k, v in ctx.profile_read().items() if v[1]}
    ctx.profile(False)
    print(fn.__name__, {k: f"{ms / n:.3f} ms x {n}" for k, (ms, n) in pr.items()}, flush=True)
print("workspace bytes:", ctx.workspace_bytes(), flush=True)
ctx.check(st)
ctx.close()
sys.exit(0 if same else 1)
