"""Cost of the aerosol-free Chou-Suarez SW fluxes at 100 000 columns x 72 layers, fp32, 60 % cloudy columns with aerosols (the columns of
`bench.py --scheme sorad`, drawn from a base of 4000), device pointers:
(a) one geosrad_sorad_na_dev call; (b) what a caller had to do without it: geosrad_sorad_dev with the aerosols, then geosrad_sorad_dev
with three arrays of zeros; (c) the driver-level pair: geosrad_sw_driver_chou_na_dev against two geosrad_sw_driver_chou_dev calls, the
second with the aerosol inputs NULL; (p) the plain geosrad_sorad_dev.  The variants alternate, REPS times each after a warm-up of all;
times from device events around each call.  (a) and (b) must give the same bits.  geosrad_profile gives the kernel slots.
With `plain` as the first argument only (p) is timed (for a library without the new entry points: GEOSRAD_LIB)."""
import sys
import numpy as np
import torch
sys.path.insert(0, ".")
from geosradiation_gridcomp_amd import gridcomp as G
from geosradiation_gridcomp_amd import synth
from geosradiation_gridcomp_amd.api import Context

ONLY_PLAIN = len(sys.argv) > 1 and sys.argv[1] == "plain"
N, LM, REPS, BASE = 100_000, 72, 20, 4000
inp = synth.make_columns(BASE, LM, start=0, cloudy_frac=0.6, aerosol=True)
cs = synth.chou_sw_inputs(inp, aerosol=True)
f = synth.geos_chou_sw_fields(inp, aerosol=True)
pick = np.random.default_rng(23).integers(0, BASE, N)
ctx = Context(4)
dt, tdt = ctx.dtype, torch.float32
IN = ("cosz", "pl", "ta", "wa", "oa", "cwc", "fcld", "reff", "taua", "ssaa", "asya", "rsuvbm", "rsuvdf", "rsirbm", "rsirdf")
dev = lambda a: torch.from_numpy(np.ascontiguousarray(np.asarray(a)[..., pick], dtype=dt)).cuda()
d = {k: dev(cs[k]) for k in IN}
zero = torch.zeros_like(d["taua"])
shape = lambda k: (LM + 1, N) if k in ("flx", "flc", "flxu", "flcu") else ((8, N) if "band" in k else (N,))
OUT = ("flx", "flc", "flxu", "flcu", "fdiruv", "fdifuv", "fdirpar", "fdifpar", "fdirir", "fdifir", "flx_sfc_band", "drband", "dfband")
mk = lambda: {k: torch.empty(shape(k), dtype=tdt, device="cuda") for k in OUT}
o1, o2 = mk(), mk()
na = {k + "_na": torch.empty(shape(k), dtype=tdt, device="cuda") for k in ("flx", "flc", "flxu", "flcu", "flx_sfc_band")}
st = torch.cuda.current_stream().cuda_stream
pin = {k: v.data_ptr() for k, v in d.items()}
pz = dict(pin, taua=zero.data_ptr(), ssaa=zero.data_ptr(), asya=zero.data_ptr())
tail = (cs["co2"], cs["ict"], cs["icb"], cs["hk_uv"], cs["hk_ir"])
P = lambda base, o: {**base, **{k: v.data_ptr() for k, v in o.items()}}
# the driver's fields
fld = {k: dev(f[k]) for k in G.SWC_IN}
drows = lambda k: 8 if "BAND" in k else (LM + 1 if k.startswith("FS") else 1)
dmk = lambda names: {k: torch.empty((drows(k), N), dtype=tdt, device="cuda") for k in names}
do1, do2 = dmk(G.SWC_OUT), dmk(G.SWC_OUT)
dfp = {k: v.data_ptr() for k, v in fld.items()}
dtail = (G.swc_consts(co2=f["CO2"]), f["LCLDMH"], f["LCLDLM"], f["HK_UV"], f["HK_IR"])


def plain():
    ctx.sorad_dev(st, N, LM, 8, P(pin, o1), *tail, do_drfband=True)


def twice():
    ctx.sorad_dev(st, N, LM, 8, P(pin, o1), *tail, do_drfband=True)
    ctx.sorad_dev(st, N, LM, 8, P(pz, o2), *tail, do_drfband=False)


def shared():
    ctx.sorad_na_dev(st, N, LM, 8, P(pin, o1), *tail, do_drfband=True, na_ptr={k: v.data_ptr() for k, v in na.items()})


def driver_twice():
    ctx.sw_driver_chou_dev(st, N, LM, P(dfp, do1), *dtail, do_drfband=True)
    ctx.sw_driver_chou_dev(st, N, LM, P({k: v for k, v in dfp.items() if k not in ("TAUA", "SSAA", "ASYA")}, do2), *dtail, do_drfband=False)


def driver_shared():
    ctx.sw_driver_chou_na_dev(st, N, LM, P(dfp, do1), *dtail, do_drfband=True, na_ptr={k: v.data_ptr() for k, v in dna.items()})


same = True
if ONLY_PLAIN:
    fns = (plain,)
else:
    dna = dmk(G.SWCNA_OUT)
    fns = (plain, twice, shared, driver_twice, driver_shared)
    twice(); ctx.check(st)
    a = {k: v.clone() for k, v in o1.items()}; a2 = {k: v.clone() for k, v in o2.items()}
    shared(); ctx.check(st)
    same = all(torch.equal(o1[k], a[k]) for k in OUT) and all(torch.equal(na[k + "_na"], a2[k]) for k in ("flx", "flc", "flxu", "flcu", "flx_sfc_band"))
    print("outputs of (a) and (b) bitwise equal:", same, flush=True)
    driver_twice(); ctx.check(st)
    b = {k: v.clone() for k, v in do1.items()}; b2 = {k: v.clone() for k, v in do2.items()}
    driver_shared(); ctx.check(st)
    dsame = all(torch.equal(do1[k], b[k]) for k in G.SWC_OUT) and all(torch.equal(dna[k], b2[k[:-2]]) for k in G.SWCNA_OUT)
    print("driver pair bitwise equal:", dsame, flush=True)
    same = same and dsame
for fn in fns:
    fn()
torch.cuda.synchronize()
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
for fn in fns:
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
