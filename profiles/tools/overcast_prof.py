"""100 000 columns x 72 layers, cloudy_frac 0.6: irrad and sorad through the _dev entry points, default then OVERCAST, fp32 and fp64,
3 launches each after one warm-up.  Run under rocprofv3 --kernel-trace --stats; also prints host-clock step times (synchronised)."""
import sys, time
import numpy as np
import torch
sys.path.insert(0, ".")
from geosradiation_gridcomp_amd import synth
from geosradiation_gridcomp_amd.api import Context
from tests.test_chou_overcast import _irrad_dev, _sorad_dev

m = int(sys.argv[1]) if len(sys.argv) > 1 else 100_000
inp = synth.make_columns(m, 72, start=11, cloudy_frac=0.6, aerosol=True)
ch, cs = synth.chou_lw_inputs(inp, aerosol=True), synth.chou_sw_inputs(inp, aerosol=True)
for rk in (4, 8):
    ctx = Context(rk)
    res = {}
    for oc in (False, True):
        ctx.set_overcast(irrad=oc, sorad=oc)
        for name, fn, d in (("irrad", _irrad_dev, ch), ("sorad", _sorad_dev, cs)):
            fn(ctx, d)                                   # warm-up
            torch.cuda.synchronize()
            t = []
            for _ in range(3):
                t0 = time.perf_counter(); out = fn(ctx, d); t.append(time.perf_counter() - t0)
            res[(oc, name)] = out
            print(f"r{rk} {'overcast' if oc else 'default '} {name}: call incl. copies {1e3 * min(t):.2f} ms", flush=True)
    for name, key in (("irrad", "flxu"), ("sorad", "flx")):
        a, b = res[(False, name)][key], res[(True, name)][key]
        print(f"r{rk} {name}: max |overcast - default| {key} = {float(np.abs(a.astype(np.float64) - b).max()):.3e}", flush=True)
    ctx.close()
