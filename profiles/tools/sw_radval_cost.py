"""Cost of the SOLAR_RADVAL diagnostics of rrtmg_sw at 97 200 columns x 72 layers, fp32, 60 % cloudy columns, device entry points:
(a) geosrad_rrtmg_sw_dev, (b) geosrad_rrtmg_sw_radval_dev on the same device arrays.  The two alternate, REPS times each after a warm-up of
both; times from device events around each call.  With `trace` as the argument nothing is timed: three calls of each for a rocprofv3
--kernel-trace --stats run of its own (k_mcica<., 2, true> against k_mcica<., 2, false>, k_sw_radval)."""
import sys
import numpy as np
import torch
sys.path.insert(0, ".")
from geosradiation_gridcomp_amd import synth
from geosradiation_gridcomp_amd.api import Context

N, LM, REPS, BASE = 97_200, 72, 10, 4000
trace_only = len(sys.argv) > 1 and sys.argv[1] == "trace"
inp = synth.make_columns(BASE, LM, start=0, cloudy_frac=0.6, aerosol=True)
pick = np.random.default_rng(23).integers(0, BASE, N)
ctx = Context(4)
names = ["coszen", "play", "plev", "tlay", "h2ovmr", "o3vmr", "co2vmr", "ch4vmr", "o2vmr", "cldf", "ciwp", "clwp", "rei", "rel", "zm", "alat",
         "tauaer_sw", "ssaaer_sw", "asmaer_sw", "asdir", "asdif", "aldir", "aldif"]
t = {k: torch.from_numpy(np.ascontiguousarray(np.asarray(inp[k])[..., pick], dtype=ctx.dtype)).cuda() for k in names}
for k in ("swuflx", "swdflx", "swuflxc", "swdflxc"):
    t[k] = torch.zeros((LM + 1, N), dtype=torch.float32, device="cuda")
for k in ("nirr", "nirf", "parr", "parf", "uvrr", "uvrf", "cotdtp", "cotdhp", "cotdmp", "cotdlp", "cotntp", "cotnhp", "cotnmp", "cotnlp"):
    t[k] = torch.zeros(N, dtype=torch.float32, device="cuda")
t["fswband"] = torch.zeros((14, N), dtype=torch.float32, device="cuda")
t["clearCounts_sw"] = torch.zeros((4, N), dtype=torch.int32, device="cuda")
t["radval"] = torch.zeros((120, N), dtype=torch.float32, device="cuda")
ptr = {k: v.data_ptr() for k, v in t.items()}
st = torch.cuda.current_stream().cuda_stream
args = (st, N, LM, 1361.0, 1.0, 0, ptr, 3, 1, inp["dyofyr"], 10, inp["cloudLM"], inp["cloudMH"])


def plain():
    ctx.rrtmg_sw_dev(*args)


def radval():
    ctx.rrtmg_sw_radval_dev(*args)


for fn in (plain, radval):
    fn(); torch.cuda.synchronize()
print("workspace bytes with the diagnostics:", ctx.workspace_bytes(), flush=True)
if trace_only:
    for _ in range(3):
        plain(); radval()
    torch.cuda.synchronize()
    sys.exit(0)
times = {"plain": [], "radval": []}
for _ in range(REPS):
    for fn in (plain, radval):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record(); torch.cuda.synchronize()
        times[fn.__name__].append(e0.elapsed_time(e1))
for k, v in times.items():
    v = np.array(v)
    print(f"{k}: median {np.median(v):.3f} ms, min {v.min():.3f}, max {v.max():.3f}, std {v.std():.3f} over {REPS} calls", flush=True)
ctx.close()
