"""GPU: swobio_driver.F90, a Fortran caller of the SOLAR TO OBIO conversion of UPDATE_EXPORT (GEOS_SolarGridComp.F90:7584-7737): `call
sw_update_obio` (module geosrad_gridcomp) on device fields.  Same library, same inputs: the same bits as the Python mirror of the entry
point, which tests/test_gpu_sw_obio.py holds against the restatement of the Fortran."""
import os
import subprocess
import numpy as np
import pytest
from tests.conftest import ROOT

pytestmark = pytest.mark.gpu
FDIR = os.path.join(ROOT, "geosradiation_gridcomp_amd", "fortran")


@pytest.mark.parametrize("kind", ["r8", "r4"])
def test_fortran_solar_to_obio_on_device_fields(tmp_path, kind, gpu_ctx):
    import torch
    from geosradiation_gridcomp_amd import gridcomp as G
    exe = os.path.join(FDIR, "bin", f"swobio_driver_{kind}")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-s", "-C", FDIR])
    ncol = 777
    rng = np.random.default_rng(9)
    slr = rng.uniform(0, 1300, ncol).astype(np.float32)
    slr[rng.uniform(size=ncol) < 0.3] = 0.0
    xr = rng.uniform(0, 1, (14, ncol)).astype(np.float32)
    xf = rng.uniform(0, 1, (14, ncol)).astype(np.float32)
    fin, fout = tmp_path / "in.bin", tmp_path / "out.bin"
    with open(fin, "wb") as fh:
        np.array([ncol], dtype=np.int32).tofile(fh)
        slr.tofile(fh); xr.tofile(fh); xf.tofile(fh)
    env = dict(os.environ, GEOSRAD_DATA=os.path.join(ROOT, "geosradiation_gridcomp_amd", "data"))
    subprocess.check_call([exe, str(fin), str(fout)], env=env)
    drobio, dfobio, dr2 = np.fromfile(fout, dtype=np.float64).reshape(3, 33, ncol)
    # the Python call
    ctx = gpu_ctx[4 if kind == "r4" else 8]
    dt = ctx.dtype
    st = torch.cuda.current_stream().cuda_stream
    t = [torch.from_numpy(v.astype(dt)).cuda() for v in (slr, xr, xf)]
    o = [torch.full((33, ncol), -7.0, dtype=t[0].dtype, device="cuda") for _ in range(2)]
    ctx.sw_update_obio_dev(st, ncol, G.OBIO_RRTMG, t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), o[0].data_ptr(), o[1].data_ptr())
    ctx.check(st)
    np.testing.assert_array_equal(drobio, o[0].cpu().numpy().astype(np.float64))
    np.testing.assert_array_equal(dfobio, o[1].cpu().numpy().astype(np.float64))
    np.testing.assert_array_equal(dr2, dfobio)          # the second call: DROBIO from the diffuse internal, DFOBIO not associated
    assert (drobio[:, slr > 0] > 0).all() and (drobio[:, slr == 0] == 0).all() and drobio.max() > 100.0
