"""fortran/lidar_driver.F90 - a caller of the external subroutine `scops` (fortran/satsim_shims.F90) and of the batched
`geosrad_lidar_simulator` (fortran/lidar_shims.F90), made the way a Fortran model makes its calls: no interface block, explicit-shape
arrays.  CPU: the demo builds and links in both kinds.  GPU (pytest -m gpu): every value it writes equals the C entry points'
(Context.scops / Context.lidar) bit for bit."""
import os
import subprocess

import numpy as np
import pytest

from tests import satsim_util as U
from tests import satsim_misr_modis_util as M
from tests import lidar_util as LU
from tests.conftest import ROOT

NPTS, NLEV, NCOL, OVERLAP, ICE = 70, 24, 7, 3, 1
FDIR = os.path.join(ROOT, "geosradiation_gridcomp_amd", "fortran")


def _exe(kind):
    exe = os.path.join(FDIR, "bin", f"lidar_driver_{kind}")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-s", "-C", FDIR, os.path.join("bin", f"lidar_driver_{kind}")])
    return exe


@pytest.mark.parametrize("kind", ["r8", "r4"])
def test_fortran_demo_links(kind):
    exe = _exe(kind)
    assert os.access(exe, os.X_OK)
    nm = subprocess.run(["nm", "-D", "--undefined-only", exe], capture_output=True, text=True, check=True).stdout
    assert " geosrad_lidar" in nm and " geosrad_scops" in nm          # the shim's call arrives at the library's entry points
    src = open(os.path.join(FDIR, "lidar_shims.F90")).read()
    assert "bind(C, name='geosrad_lidar')" in src and "subroutine geosrad_lidar_simulator(" in src


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["r8", "r4"])
def test_fortran_caller_equals_the_api(tmp_path, gpu_ctx, kind):
    exe = _exe(kind)
    b = U.make_batch(NPTS, NLEV, seed=33)
    hy = LU.thicken(M.make_hydro(b), b)
    ex = LU.make_lidar_inputs(b)
    planes = [b["cc"], b["conv"], ex["p"], b["at"], ex["pplay"], hy["ql"], hy["qi"], hy["qlc"], hy["qic"], hy["rl"], hy["ri"], hy["rlc"], hy["ric"]]
    fin, fout = tmp_path / "in.bin", tmp_path / "out.bin"
    with open(fin, "wb") as fh:
        np.array([NPTS, NLEV, NCOL, OVERLAP, ICE], dtype=np.int32).tofile(fh)
        b["seed"].tofile(fh)
        for a in planes:      # (nlev, npoints) in C order is (npoints,nlev)
            a.astype(np.float32).tofile(fh)
        ex["presf"].astype(np.float32).tofile(fh); ex["land"].astype(np.float32).tofile(fh)
    env = dict(os.environ, GEOSRAD_DATA=os.path.join(ROOT, "geosradiation_gridcomp_amd", "data"))
    subprocess.check_call([exe, str(fin), str(fout)], env=env)
    raw = np.fromfile(fout, np.float64)
    ctx = gpu_ctx[4 if kind == "r4" else 8]
    frac, _ = ctx.scops(NPTS, NLEV, NCOL, b["seed"], b["cc"], b["conv"], OVERLAP)
    o = ctx.lidar(NPTS, NLEV, NCOL, ICE, ex["p"], b["at"], ex["presf"], ex["pplay"], frac, hy["ql"], hy["qi"], hy["qlc"], hy["qic"], hy["rl"], hy["ri"],
                  hy["rlc"], hy["ric"], ex["land"])
    want = [("frac_out", frac)] + [(n, o[n]) for n in ("lidarcld", "cldlayer", "cfad_sr", "parasolrefl", "pmol")]
    assert raw.size == sum(w.size for _, w in want)
    at = 0
    for name, w in want:
        np.testing.assert_array_equal(raw[at:at + w.size], w.astype(np.float64).ravel(), err_msg=name)
        at += w.size
    assert ((o["lidarcld"] > 0) & (o["lidarcld"] != ctx.dtype(LU.R_UNDEF))).sum() > 10 and (o["parasolrefl"] == ctx.dtype(LU.R_UNDEF)).any()
