"""profiles/tools/cloud_top_shares.py [ncol nlay cloudy_frac]: how much of a cloudy column is cloudy, counted on the CPU (no GPU needed).
The cloudy columns of synth.make_columns in partition order (input order, the cloud-free ones taken out), in waves of 64 lanes:
  - (column, layer) cells with cloud fraction,
  - layers below a column's own cloud top (colcloudy = 1 + the highest layer with cldf > 0),
  - layers below the wave's highest cloud top (where the band kernels' loops are split),
  - (wave, layer) pairs in which any lane has cloud fraction.
The last two bound what the general (cloudy) layer bodies of k_sw_reform / k_lw_bands have to run."""
import os
import sys
import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
from geosradiation_gridcomp_amd import synth  # noqa: E402


def shares(cldf, wave=64):
    nlay = cldf.shape[0]
    has = cldf > 0
    cloudy = has.any(axis=0)
    has = has[:, cloudy]                                    # the partition keeps the input order within a class
    n = has.shape[1]
    top = np.where(has.any(axis=0), nlay - np.argmax(has[::-1], axis=0), 0)       # colcloudy
    nw = (n + wave - 1) // wave
    pad = nw * wave - n
    topw = np.pad(top, (0, pad)).reshape(nw, wave).max(axis=1)
    lanes = np.full(nw, wave); lanes[-1] = wave - pad
    anyw = np.pad(has, ((0, 0), (0, pad))).reshape(nlay, nw, wave).any(axis=2)
    return dict(ncloudy=n, cells=has.mean(), own_top=top.mean() / nlay, own_top_layers=top.mean(),
                wave_top=(topw * lanes).sum() / (n * nlay), wave_top_layers=(topw * lanes).sum() / n,
                wave_layer_pairs=(anyw * lanes[None, :]).sum() / (n * nlay))


if __name__ == "__main__":
    ncol, nlay, frac = (int(sys.argv[1]), int(sys.argv[2]), float(sys.argv[3])) if len(sys.argv) > 3 else (97200, 72, 0.6)
    inp = synth.make_columns(ncol, nlay, cloudy_frac=frac, aerosol=True)
    s = shares(inp["cldf"])
    print(f"{ncol} columns x {nlay} layers, cloudy_frac {frac}: {s['ncloudy']} cloudy columns")
    print(f"cells with cldf > 0 among the cloudy columns          {100 * s['cells']:.1f} %")
    print(f"layers below a column's own cloud top (mean {s['own_top_layers']:.1f})      {100 * s['own_top']:.1f} %")
    print(f"layers below the wave's highest cloud top (mean {s['wave_top_layers']:.1f})  {100 * s['wave_top']:.1f} %")
    print(f"(wave, layer) pairs in which any lane has cloud fraction {100 * s['wave_layer_pairs']:.1f} %")
