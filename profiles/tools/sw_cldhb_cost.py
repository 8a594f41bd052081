"""Cost of the heartbeat McICA cloud fractions (geosrad_sw_update_cldhb_dev) at a C360 tile's per-GPU share, 97 200 columns x 72 layers,
60 % of the columns cloudy, ih = 1, fp32 and fp64 (profiles/r08_sw_cldhb.md).

  python profiles/tools/sw_cldhb_cost.py            time per call (HIP events, median and spread of REPS calls after warm-up): the entry
                                                    point with and without the compaction of cloudy columns, and what a caller had
                                                    before it: the same preparation in torch + geosrad_mcica_dev with 112 sub-columns on
                                                    the same columns (without the host-side clearCounts and its copy)
  python profiles/tools/sw_cldhb_cost.py once RK    three calls of the entry point in real kind RK, for a rocprofv3 run
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from geosradiation_gridcomp_amd.api import Context      # noqa: E402
from geosradiation_gridcomp_amd import gridcomp as G    # noqa: E402
from tests import sw_cldhb_util as U                    # noqa: E402

N, LM, DOY, REPS = 97200, 72, 200, 20


def fields():
    base, mh, ml = U.make_fields(4050, LM, seed=11, clear=0.4)
    pick = np.random.default_rng(5).integers(0, 4050, N)
    return {k: np.ascontiguousarray(v[..., pick]) for k, v in base.items()}, mh, ml


def timed(fn, reps=REPS):
    fn(); fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    ms = np.array(ms)
    return float(np.median(ms)), float(ms.min()), float(ms.max())


def torch_prepare(t, tdt):
    """SOL:7133-7161 as a caller would write it in torch (zmid by the same recurrence, layer by layer)"""
    ple, tt = t["PLE"], t["T"]
    plmid = 0.5 * (ple[:-1] + ple[1:])
    play = plmid / 100.
    cfac = 102. * (ple[1:] - ple[:-1])
    ciwp, clwp = cfac * t["QI"], cfac * t["QL"]
    tlev = (tt[:-1] * cfac[1:] + tt[1:] * cfac[:-1]) / (cfac[1:] + cfac[:-1])
    zmid = torch.zeros_like(tt)
    for k in range(LM - 2, -1, -1):
        zmid[k] = zmid[k + 1] + (U.RGAS * tlev[k]) / U.GRAV * (plmid[k + 1] - plmid[k]) / ple[k + 1]
    return dict(zm=zmid, play=play, ciwp=ciwp, clwp=clwp)


def main():
    f, mh, ml = fields()
    once = len(sys.argv) > 2 and sys.argv[1] == "once"
    st = torch.cuda.current_stream().cuda_stream
    print(f"{N} x {LM}, cloudy columns {(f['FCLD'] > 0).any(axis=0).mean():.3f}, lcldmh {mh}, lcldlm {ml}", flush=True)
    for rk in ([int(sys.argv[2])] if once else [4, 8]):
        ctx = Context(rk, tables=False)
        ctx.set_inhomogeneity(1)
        tdt = torch.float32 if rk == 4 else torch.float64
        t = {k: torch.from_numpy(np.ascontiguousarray(f[k], dtype=ctx.dtype)).cuda() for k in G.SWHB_IN}
        o = {k: torch.zeros(N, dtype=tdt, device="cuda") for k in G.SWHB_OUT}
        ptr = {k: v.data_ptr() for k, v in {**t, **o}.items()}
        call = lambda: ctx.sw_update_cldhb_dev(st, N, LM, mh, ml, DOY, ptr)
        if once:
            for _ in range(3):
                call()
            ctx.check(st)
            ctx.close()
            continue
        res = {}
        for compact in ("1", "0"):
            os.environ["GEOSRAD_SWHB_COMPACT"] = compact
            res[compact] = timed(call)
            keep = torch.stack([o[k] for k in G.SWHB_OUT]).clone()
            res["out" + compact] = keep
        del os.environ["GEOSRAD_SWHB_COMPACT"]
        assert torch.equal(res["out1"], res["out0"])
        print(f"r{rk}: sw_update_cldhb_dev per call [ms] median (min .. max) of {REPS}: compacted {res['1'][0]:.3f} ({res['1'][1]:.3f} .. {res['1'][2]:.3f}); "
              f"not compacted {res['0'][0]:.3f} ({res['0'][1]:.3f} .. {res['0'][2]:.3f}); CLDTT mean {float(o['CLDTT'].mean()):.4f}", flush=True)
        # the parent's path: torch preparation + the materialising generator on the same columns
        d = dict(alat=t["LATS"], cldf=t["FCLD"])
        d["cldy_stoch"] = torch.zeros((N, U.NSUB, LM), dtype=torch.int32, device="cuda")
        d["ciwp_stoch"] = torch.zeros((N, U.NSUB, LM), dtype=tdt, device="cuda")
        d["clwp_stoch"] = torch.zeros((N, U.NSUB, LM), dtype=tdt, device="cuda")

        def parent():
            p = torch_prepare(t, tdt)
            q = {**d, **p}
            ctx.generate_stochastic_clouds_dev(st, N, U.NSUB, LM, {k: v.data_ptr() for k, v in q.items()}, DOY, 1e-20, seed_order=U.SEED_ORDER)
            return p
        pm = timed(parent, reps=8)
        gen = timed(lambda p=parent(): ctx.generate_stochastic_clouds_dev(st, N, U.NSUB, LM, {k: v.data_ptr() for k, v in {**d, **p}.items()}, DOY,
                                                                        1e-20, seed_order=U.SEED_ORDER), reps=8)
        print(f"r{rk}: torch preparation + geosrad_mcica_dev(112) per call [ms]: {pm[0]:.3f} ({pm[1]:.3f} .. {pm[2]:.3f}); the generator alone "
              f"{gen[0]:.3f} ({gen[1]:.3f} .. {gen[2]:.3f}); ratio to the fused call {pm[0] / res['1'][0]:.2f} (generator alone {gen[0] / res['1'][0]:.2f})", flush=True)
        ctx.check(st)
        del d
        torch.cuda.empty_cache()
        ctx.close()


if __name__ == "__main__":
    main()
