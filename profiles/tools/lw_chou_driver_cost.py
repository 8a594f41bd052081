"""Cost of the Chou-Suarez branch of LW_Driver at 100 000 columns x 72 layers, fp32, 60 % cloudy columns with aerosols:
(a) geosrad_lw_driver_chou_dev; (b) the way open to a caller without it: the same preparation as torch device operations into staged
CWC / REFF / surface arrays, geosrad_irrad_dev, geosrad_lw_chou_post_dev, the diagnostics as torch operations.  The two alternate, REPS
times each after a warm-up of both; times from device events around each call.  geosrad_profile gives the share of the preparation kernel
and of k_chou_bands in (a) and (b).  With `trace` as the argument nothing is timed: three calls of (a) for a rocprofv3 --kernel-trace
--stats run of its own."""
import sys
import numpy as np
import torch
sys.path.insert(0, ".")
from geosradiation_gridcomp_amd import gridcomp as G
from geosradiation_gridcomp_amd import synth
from geosradiation_gridcomp_amd.api import Context

N, LM, REPS, BASE = 100_000, 72, 20, 4000
trace_only = len(sys.argv) > 1 and sys.argv[1] == "trace"
inp = synth.make_columns(BASE, LM, start=0, cloudy_frac=0.6, aerosol=True)
f = synth.geos_chou_lw_fields(inp, aerosol=True)
pick = np.random.default_rng(23).integers(0, BASE, N)
ctx = Context(4)
dt, tdt = ctx.dtype, torch.float32
fld = {k: torch.from_numpy(np.ascontiguousarray(f[k][..., pick], dtype=dt)).cuda() for k in G.LWK_IN}
aer0 = {k: fld[k].clone() for k in ("TAUA", "SSAA", "ASYA")}            # in-out: restored before every call, outside the timed window
consts = G.lwk_consts(co2=f["CO2"])
mh, lmid = f["LCLDMH"], f["LCLDLM"]
shape = lambda k: (LM + 1, N) if k in G.LWK_OUT[:9] + G.LWK_OUT[10:17] else (LM, N) if k == "TAUIR" else (10, LM, N) if k == "TAUDIAG" else (N,)
want = [k for k in G.LWK_OUT if k not in ("T2M", "TAUDIAG")]            # what a GridComp asks for
out = {k: torch.empty(shape(k), dtype=tdt, device="cuda") for k in want}
st = torch.cuda.current_stream().cuda_stream
undef = torch.tensor(consts[2], dtype=tdt, device="cuda")


def restore():
    for k, v in aer0.items():
        fld[k].copy_(v)


def driver():
    ptr = {k: v.data_ptr() for k, v in fld.items()}
    ptr.update({k: v.data_ptr() for k, v in out.items()})
    ctx.lw_driver_chou_dev(st, N, LM, ptr, consts, True, mh, lmid)


stg = {}


def staged():
    """LW_Driver's preparation, irrad, the post step and the diagnostics with what the parent commit offers"""
    T, PLE, TS = fld["T"], fld["PLE"], fld["TS"]
    t2m = T[LM - 1] * (0.5 * (1.0 + PLE[LM - 1] / PLE[LM])) ** (-consts[1])
    cwc = torch.stack([fld[q] for q in ("QI", "QL", "QR", "QS")])
    reff = torch.stack([torch.where(fld[r] == undef, torch.tensor(d, dtype=tdt, device="cuda"), fld[r]) * 1.0e6
                        for r, d in zip(("RI", "RL", "RR", "RS"), (36.e-6, 14.e-6, 50.e-6, 50.e-6))])
    fcld = fld["FCLD"].clone()                                           # FCLD = FCLD_IN (IRR:1781)
    fs = torch.ones((1, N), dtype=tdt, device="cuda"); tg = TS.reshape(1, N).clone(); tv = TS.reshape(1, N).clone()
    eg = fld["EMIS"].reshape(1, 1, N).expand(10, 1, N).contiguous()
    ev = torch.zeros((10, 1, N), dtype=tdt, device="cuda"); rv = torch.zeros((10, 1, N), dtype=tdt, device="cuda")
    if "taudiag" not in stg:
        stg["taudiag"] = torch.empty((10, LM, N), dtype=tdt, device="cuda")
    td = stg["taudiag"]
    p = dict(ple=PLE, ta=T, wa=fld["Q"], oa=fld["O3"], tb=t2m, n2o=fld["N2O"], ch4=fld["CH4"], cfc11=fld["CFC11"], cfc12=fld["CFC12"],
             cfc22=fld["HCFC22"], cwc=cwc, fcld=fcld, reff=reff, fs=fs, tg=tg, eg=eg, tv=tv, ev=ev, rv=rv, taua=fld["TAUA"], ssaa=fld["SSAA"],
             asya=fld["ASYA"], taudiag=td)
    ptr = {k: v.data_ptr() for k, v in p.items()}
    for a, b in zip(("flxu", "flcu", "flau", "flxau", "flxd", "flcd", "flad", "flxad", "dfdts", "sfcem"), G.LWK_OUT_REQUIRED):
        ptr[a] = out[b].data_ptr()
    ctx.irrad_dev(st, N, LM, ptr, consts[0], True, mh, lmid, 1, 1, 10)
    g = {k: out[k].data_ptr() for k in G.LWC_OUT}
    g.update({k: out[k].data_ptr() for k in G.LWC_IN if k != "TS"})
    g["TS"] = TS.data_ptr()
    ctx.lw_chou_post_dev(st, N, LM, g)
    tau = 0.5 * (td[2] + td[3])
    out["TAUIR"].copy_(tau)
    hit = tau > (np.float32(consts[3]) / np.float32(2.13))
    found = hit.any(dim=0)
    first = hit.to(torch.int8).argmax(dim=0, keepdim=True)
    out["CLDTMP"].copy_(torch.where(found, T.gather(0, first)[0], undef))
    out["CLDPRS"].copy_(torch.where(found, PLE.gather(0, first)[0], undef))
    out["TSREFF"].copy_(TS); out["DSFDTS0"].copy_(-out["DFDTS"][LM]); out["SFCEM0"].copy_(out["SFCEM_INT"])
    out["LWS0"].copy_(out["FLX_INT"][LM] + out["SFCEM_INT"])


if trace_only:
    for _ in range(3):
        restore(); driver()
    torch.cuda.synchronize()
    sys.exit(0)

ref = {}
for fn in (driver, staged):                                              # warm-up of both, and the two must agree
    restore(); fn(); torch.cuda.synchronize()
    ref[fn.__name__] = {k: v.clone() for k, v in out.items()}
same = all(torch.equal(ref["driver"][k], ref["staged"][k]) for k in want)
print("outputs of (a) and (b) bitwise equal (torch's pow in T2M may differ from the kernel's in the last bit):", same, flush=True)
if not same:
    for k in want:
        if not torch.equal(ref["driver"][k], ref["staged"][k]):
            print("  differs:", k, float((ref["driver"][k] - ref["staged"][k]).abs().max()), flush=True)
times = {"driver": [], "staged": []}
for _ in range(REPS):
    for fn in (driver, staged):
        restore(); torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record(); torch.cuda.synchronize()
        times[fn.__name__].append(e0.elapsed_time(e1))
for k, v in times.items():
    v = np.array(v)
    print(f"{k}: median {np.median(v):.3f} ms, min {v.min():.3f}, max {v.max():.3f}, std {v.std():.3f} over {REPS} calls", flush=True)
for fn in (driver, staged):
    ctx.profile(True)
    for _ in range(5):
        restore(); fn()
    torch.cuda.synchronize()
    pr = {k: v for k, v in ctx.profile_read().items() if v[1]}
    ctx.profile(False)
    print(fn.__name__, {k: f"{ms / n:.3f} ms x {n}" for k, (ms, n) in pr.items()}, flush=True)
# bytes the fused preparation must move: PLE (LM+1) + T Q O3 N2O CH4 CFC11 CFC12 HCFC22 FCLD QI..QS RI..RS (17 LM) read, 22 fields x (LM+1) written
byts = N * ((LM + 1) + 17 * LM + 22 * (LM + 1)) * 4
print(f"preparation kernel: {byts / 1e9:.4f} GB to move", flush=True)
print("workspace bytes:", ctx.workspace_bytes(), flush=True)
ctx.close()
