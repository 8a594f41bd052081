"""GPU (pytest -m gpu): fortran/misr_driver.F90 - a caller of the external subroutines `scops` and `MISR_simulator` with the reference's
argument lists (fortran/satsim_shims.F90, fortran/misr_modis_shims.F90), made the way cosp.F90:397 and cosp_misr_simulator.F90:72-74 make
theirs.  Every value equals the C entry points' (Context.scops / Context.misr) bit for bit, and the numpy restatement."""
import os
import subprocess

import numpy as np
import pytest

from tests import satsim_util as U
from tests import satsim_misr_modis_util as M
from tests.conftest import ROOT

NPTS, NLEV, NCOL, OVERLAP = 72, 24, 7, 3          # 72: the last point is dark


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["r8", "r4"])
def test_fortran_caller_equals_the_api(tmp_path, gpu_ctx, kind):
    fdir = os.path.join(ROOT, "geosradiation_gridcomp_amd", "fortran")
    exe = os.path.join(fdir, "bin", f"misr_driver_{kind}")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-s", "-C", fdir, os.path.join("bin", f"misr_driver_{kind}")])
    b = U.make_batch(NPTS, NLEV, seed=32)
    b.update(M.make_hydro(b))
    fin, fout = tmp_path / "in.bin", tmp_path / "out.bin"
    with open(fin, "wb") as fh:
        np.array([NPTS, NLEV, NCOL, OVERLAP], dtype=np.int32).tofile(fh)
        b["sunlit"].tofile(fh); b["seed"].tofile(fh)
        for k in ("cc", "conv", "zfull", "at", "dtau_s", "dtau_c"):      # (nlev, npoints) in C order is (npoints,nlev)
            b[k].astype(np.float32).tofile(fh)
        np.array([M.MISSING], np.float32).tofile(fh)
    env = dict(os.environ, GEOSRAD_DATA=os.path.join(ROOT, "geosradiation_gridcomp_amd", "data"))
    subprocess.check_call([exe, str(fin), str(fout)], env=env)
    raw = np.fromfile(fout, np.float64)

    ctx = gpu_ctx[4 if kind == "r4" else 8]
    missing = float(ctx.dtype(np.float32(M.MISSING)))                  # the caller's missing_value is a default real read from a real(4)
    frac, _ = ctx.scops(NPTS, NLEV, NCOL, b["seed"], b["cc"], b["conv"], OVERLAP)
    o = ctx.misr(NPTS, NLEV, NCOL, b["sunlit"], b["zfull"], b["at"], b["dtau_s"], b["dtau_c"], frac, missing)
    R = ctx.dtype
    want = [("frac_out", frac)] + [(n, o[n]) for n in M.MISR_OUT]
    head = sum(w.size for _, w in want)
    # the batched geosrad_modis_simulator call the driver makes after MISR: its pressures go through the caller's own exp, which is not
    # numpy's to the bit, so what is asserted here is that the call arrives - shapes, the wrapper's rules, the histogram holding every
    # retrieved cloud once; the values are tests/test_gpu_modis.py's
    mm, mh = raw[head:head + 17 * NPTS].reshape(17, NPTS), raw[head + 17 * NPTS:].reshape(7, 7, NPTS)
    raw = raw[:head]
    dark = b["sunlit"] <= 0
    assert (mm[:, dark] == float(R(M.R_UNDEF))).all() and (mh[:, :, dark] == float(R(M.R_UNDEF))).all() and (mh[:, 0, :] == float(R(M.R_UNDEF))).all()
    lit_cf = mm[0][~dark]
    assert ((lit_cf >= 0) & (lit_cf <= 1)).all() and (lit_cf > 0).sum() > 10 and (mm[2][~dark] == 0).all()          # liquid only: no ice cloud
    assert np.allclose(mh[:, 1:, :][:, :, ~dark].sum(axis=(0, 1)), lit_cf, atol=1e-6)                                  # every retrieved cloud is in one cell
    assert raw.size == sum(w.size for _, w in want)
    at = 0
    for name, w in want:
        np.testing.assert_array_equal(raw[at:at + w.size], w.astype(np.float64).ravel(), err_msg=name)
        at += w.size
    r = M.misr(b["sunlit"], b["zfull"], b["at"], b["dtau_s"], b["dtau_c"], frac.astype(np.uint8), missing, ctx.dtype)
    for n in M.MISR_OUT:
        np.testing.assert_array_equal(o[n], r[n], err_msg=n)
    assert (o["MISR_cldarea"] > 0).sum() > 10 and o["MISR_mean_ztop"][-1] == ctx.dtype(missing) and b["sunlit"][-1] != 1
