"""GPU (pytest -m gpu): fortran/satsim_driver.F90 - a caller of the external subroutines `scops` and `icarus` with the reference's argument
lists (fortran/satsim_shims.F90), made the way cosp.F90:397 and cosp_isccp_simulator.F90:74-80 make theirs.  Every value equals the C entry
points' (Context.scops / Context.icarus) bit for bit."""
import os
import subprocess

import numpy as np
import pytest

from tests import satsim_util as U
from tests.conftest import ROOT

NPTS, NLEV, NCOL = 70, 24, 7
OPTS = (3, 1, 2)            # overlap, top_height, top_height_direction: the GEOS settings


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["r8", "r4"])
def test_fortran_callers_equal_the_api(tmp_path, gpu_ctx, kind):
    fdir = os.path.join(ROOT, "geosradiation_gridcomp_amd", "fortran")
    exe = os.path.join(fdir, "bin", f"satsim_driver_{kind}")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-s", "-C", fdir, os.path.join("bin", f"satsim_driver_{kind}")])
    b = U.make_batch(NPTS, NLEV, seed=31)
    fin, fout = tmp_path / "in.bin", tmp_path / "out.bin"
    with open(fin, "wb") as fh:
        np.array([NPTS, NLEV, NCOL, *OPTS], dtype=np.int32).tofile(fh)
        b["sunlit"].tofile(fh); b["seed"].tofile(fh)
        for k in ("pfull", "phalf", "qv", "cc", "conv", "dtau_s", "dtau_c", "at", "dem_s", "dem_c", "skt"):      # (nlev, npoints) in C order is (npoints,nlev)
            b[k].astype(np.float32).tofile(fh)
        np.array([U.EMSFC_LW], np.float32).tofile(fh)
    env = dict(os.environ, GEOSRAD_DATA=os.path.join(ROOT, "geosradiation_gridcomp_amd", "data"))
    subprocess.check_call([exe, str(fin), str(fout)], env=env)
    with open(fout, "rb") as fh:
        seed = np.fromfile(fh, np.int32, NPTS)
        raw = np.fromfile(fh, np.float64)

    ctx = gpu_ctx[4 if kind == "r4" else 8]
    emsfc = float(ctx.dtype(np.float32(U.EMSFC_LW)))                  # the caller's emsfc_lw is a default real read from a real(4)
    frac, after = ctx.scops(NPTS, NLEV, NCOL, b["seed"], b["cc"], b["conv"], OPTS[0])
    o = ctx.icarus(NPTS, b["sunlit"], NLEV, NCOL, b["pfull"], b["phalf"], b["qv"], b["cc"], b["conv"], b["dtau_s"], b["dtau_c"], OPTS[1], OPTS[2], OPTS[0],
                   frac, b["skt"], emsfc, b["at"], b["dem_s"], b["dem_c"])
    np.testing.assert_array_equal(seed, after)
    want = [("frac_out", frac)] + [(n, o[n]) for n in U.ICARUS_OUT]
    assert raw.size == sum(w.size for _, w in want)
    at = 0
    for name, w in want:
        np.testing.assert_array_equal(raw[at:at + w.size], w.astype(np.float64).ravel(), err_msg=name)
        at += w.size
    rm, rs = U.scops(b["seed"], b["cc"], b["conv"], OPTS[0], NCOL, ctx.dtype)
    assert np.array_equal(frac, rm.astype(ctx.dtype)) and np.array_equal(after, rs) and (frac > 0).sum() > 50 and (o["boxptop"] > 0).sum() > 20
