"""Cost of the daytime gather / scatter of SORADCORE's SW branch on a 97 200 x 72 tile, fp32, 60 % cloudy columns with aerosols, lit
fraction 0.5 and 1.0, for both GridComp drivers:
  route A  geosrad_lit_pack_dev of every import, the packed driver (geosrad_sw_driver_rrtmg_dev / _chou_dev), geosrad_lit_unpack_dev of every result
  route B  geosrad_sw_driver_rrtmg_lit_dev / geosrad_sw_driver_chou_lit_dev on the tile
Without arguments: for every (driver, lit fraction) the two routes alternate REPS times after a warm-up of both, timed by device events
around a whole route; then the bytes of the packed twins route A needs and the device memory each route's context holds after its first
call (a context per route; hipMemGetInfo before the context is created and after the call, every tensor of the tool allocated before:
tables, solver workspace and driver buffers, also those geosrad_workspace_bytes does not count).
  python profiles/tools/sw_lit_cost.py trace DRIVER FRAC ROUTE    a warm-up and three untimed calls of one route, for a run of its own under
                                                                  rocprofv3 --kernel-trace --stats (DRIVER rrtmg | chou, ROUTE A | B)
  python profiles/tools/sw_lit_cost.py stats DIR                  per-kernel totals of the x_kernel_stats.csv files below DIR"""
import csv
import glob
import sys
import numpy as np

N, LM, REPS, BASE = 97_200, 72, 10, 4000


def stats(top):
    for f in sorted(glob.glob(top + "/**/*kernel_stats.csv", recursive=True)):
        rows = sorted(csv.DictReader(open(f)), key=lambda r: -float(r["TotalDurationNs"]))
        print(f, flush=True)
        for r in rows:
            if float(r["TotalDurationNs"]) < 20e3:
                continue
            print(f"  {r['Name'][:90]:90s} calls {int(r['Calls']):4d}  avg {float(r['AverageNs']) / 1e6:8.3f} ms  total {float(r['TotalDurationNs']) / 1e6:8.3f} ms")


if len(sys.argv) > 2 and sys.argv[1] == "stats":
    stats(sys.argv[2])
    sys.exit(0)

import torch
sys.path.insert(0, ".")
from geosradiation_gridcomp_amd import gridcomp as G
from geosradiation_gridcomp_amd import synth
from geosradiation_gridcomp_amd.api import Context

tdt = torch.float32
inp = synth.make_columns(BASE, LM, start=0, cloudy_frac=0.6, aerosol=True)
pick = np.random.default_rng(23).integers(0, BASE, N)
st = torch.cuda.current_stream().cuda_stream


class Case:
    def __init__(self, driver, frac, routes="AB"):
        self.driver, self.frac = driver, frac
        if driver == "rrtmg":
            f = synth.geos_sw_fields(inp); self.ins, self.outs = G.SWD_IN, G.SWD_OUT
            self.rows = lambda k: LM + 1 if k in ("FSW", "FSC", "FSWU", "FSCU", "FSWNA", "FSCNA", "FSWUNA", "FSCUNA") else (14 if k.startswith("FSWBAND") else 1)
        else:
            f = synth.geos_chou_sw_fields(inp, aerosol=True); self.ins, self.outs = G.SWC_IN, G.SWC_OUT
            self.rows = lambda k: LM + 1 if k in ("FSW", "FSC", "FSWU", "FSCU") else (8 if k in ("FSWBAND", "DRBAND", "DFBAND") else 1)
        self.f = f
        rng = np.random.default_rng(3)
        day = rng.uniform(size=N) < frac
        zth = np.where(day, f["ZT"][pick], -rng.uniform(0.01, 1.0, N)).astype(np.float32)
        self.tile = {k: torch.from_numpy(np.ascontiguousarray(f[k][..., pick], dtype=np.float32).reshape(-1, N)).cuda() for k in self.ins}
        self.tile["ZT"] = torch.from_numpy(zth.reshape(1, N)).cuda()
        self.zth = self.tile["ZT"]
        self.idx = torch.zeros(N, dtype=torch.int32, device="cuda"); self.pos = torch.zeros(N, dtype=torch.int32, device="cuda")
        self.nl = torch.zeros(1, dtype=torch.int32, device="cuda")
        n = self.nlit = int(day.sum())
        self.packed = {k: torch.empty((v.shape[0], n), dtype=tdt, device="cuda") for k, v in self.tile.items()}
        self.pout = {k: torch.empty((self.rows(k), n), dtype=tdt, device="cuda") for k in self.outs}
        self.out = {r: {k: torch.full((self.rows(k), N), -7.0, dtype=tdt, device="cuda") for k in self.outs} for r in "AB"}
        self.dark = {k: 0.0 for k in self.outs}
        self.twin_bytes = sum(v.numel() * 4 for v in self.packed.values()) + sum(v.numel() * 4 for v in self.pout.values())
        self.ctx, self.held = {}, {}
        for r in routes:                 # the context's own device memory: nothing else allocates between the two readings
            torch.cuda.synchronize()
            free0 = torch.cuda.mem_get_info()[0]
            self.ctx[r] = Context(4)
            self.ctx[r].set_inhomogeneity(1)
            if r == routes[0]:
                assert self.ctx[r].lit_index_dev(st, N, self.zth.data_ptr(), self.idx.data_ptr(), self.pos.data_ptr(), self.nl.data_ptr()) == n
            getattr(self, r)()
            torch.cuda.synchronize()
            self.held[r] = free0 - torch.cuda.mem_get_info()[0]

    def call(self, ctx, lit, n, ptr):
        f = self.f
        if self.driver == "rrtmg":
            a = (LM, 14, ptr, G.swd_consts(), 3, 1, 1361.0, 1.0, 0, int(inp["dyofyr"]), True, f["LCLDLM"], f["LCLDMH"], 1)
            if lit:
                ctx.sw_driver_rrtmg_lit_dev(st, N, n, self.idx.data_ptr(), self.pos.data_ptr(), *a, dark=self.dark)
            else:
                ctx.sw_driver_rrtmg_dev(st, n, *a)
        else:
            a = (LM, ptr, G.swc_consts(co2=f["CO2"]), f["LCLDMH"], f["LCLDLM"], f["HK_UV"], f["HK_IR"])
            if lit:
                ctx.sw_driver_chou_lit_dev(st, N, n, self.idx.data_ptr(), self.pos.data_ptr(), *a, do_drfband=True, dark=self.dark)
            else:
                ctx.sw_driver_chou_dev(st, n, *a, do_drfband=True)

    def A(self):
        ctx, n = self.ctx["A"], self.nlit
        for k, v in self.tile.items():
            ctx.lit_pack_dev(st, n, N, v.shape[0], self.idx.data_ptr(), self.nl.data_ptr(), v.data_ptr(), self.packed[k].data_ptr())
        ptr = {k: v.data_ptr() for k, v in self.packed.items()}
        ptr.update({k: v.data_ptr() for k, v in self.pout.items()})
        self.call(ctx, False, n, ptr)
        for k in self.outs:
            ctx.lit_unpack_dev(st, n, N, self.rows(k), self.pos.data_ptr(), self.pout[k].data_ptr(), self.out["A"][k].data_ptr(), default=0.0)

    def B(self):
        ptr = {k: v.data_ptr() for k, v in self.tile.items()}
        ptr.update({k: v.data_ptr() for k, v in self.out["B"].items()})
        self.call(self.ctx["B"], True, self.nlit, ptr)

    def close(self):
        for c in self.ctx.values():
            c.close()


if len(sys.argv) > 4 and sys.argv[1] == "trace":
    c = Case(sys.argv[2], float(sys.argv[3]), routes=sys.argv[4])          # its one call in there is the warm-up
    for _ in range(3):
        getattr(c, sys.argv[4])()
    torch.cuda.synchronize()
    c.close()
    sys.exit(0)

for driver in ("rrtmg", "chou"):
    for frac in (0.5, 1.0):
        c = Case(driver, frac)
        for fn in (c.A, c.B):
            fn(); torch.cuda.synchronize()
        same = all(torch.equal(c.out["A"][k], c.out["B"][k]) for k in c.outs)
        times = {"A": [], "B": []}
        for _ in range(REPS):
            for r in "AB":
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(); getattr(c, r)(); e1.record(); torch.cuda.synchronize()
                times[r].append(e0.elapsed_time(e1))
        print(f"{driver} lit {frac}: nlit {c.nlit} of {N}; outputs of A and B bitwise equal: {same}", flush=True)
        for r in "AB":
            v = np.array(times[r])
            print(f"  route {r}: median {np.median(v):.3f} ms, min {v.min():.3f}, max {v.max():.3f} over {REPS} calls; "
                  f"context holds {c.held[r] / 2**20:.1f} MiB of device memory (geosrad_workspace_bytes {c.ctx[r].workspace_bytes() / 2**20:.1f} MiB)"
                  + (f" + packed twins {c.twin_bytes / 2**20:.1f} MiB" if r == "A" else ""), flush=True)
        c.close()
        del c
        torch.cuda.empty_cache()
