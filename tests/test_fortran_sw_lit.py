"""GPU: swlit_driver.F90, a Fortran caller of the lit-aware Chou-Suarez branch of SORADCORE: `call lit_index` on ZTH, then one
`call sw_driver_chou_lit` (module geosrad_gridcomp) on the un-packed device fields (GEOS_SolarGridComp.F90:3686, PackIt :3839-3894,
SORADCORE :4484-4572, UnPackIt :6520-6580).  Same library, same inputs: the same bits as the Python mirror of the entry point."""
import os
import subprocess
import numpy as np
import pytest
from tests.conftest import ROOT

pytestmark = pytest.mark.gpu
FDIR = os.path.join(ROOT, "geosradiation_gridcomp_amd", "fortran")


@pytest.mark.parametrize("kind", ["r8", "r4"])
def test_fortran_lit_aware_chou_branch_on_device_fields(tmp_path, kind, gpu_ctx):
    import torch
    from geosradiation_gridcomp_amd import gridcomp as G
    from geosradiation_gridcomp_amd import synth
    exe = os.path.join(FDIR, "bin", f"swlit_driver_{kind}")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-s", "-C", FDIR])
    ncol, lm = 70, 72
    inp = synth.make_columns(ncol, lm, start=919, aerosol=True, cloudy_frac=0.6)
    f = synth.geos_chou_sw_fields(inp, aerosol=True)
    rng = np.random.default_rng(5)
    day = rng.uniform(size=ncol) < 0.47
    day[0] = False; day[-1] = True
    zth = np.where(day, f["ZT"], -rng.uniform(0.01, 1.0, ncol)).astype(np.float32)
    zth[7] = 0.0; day[7] = False
    f["ZT"] = zth.astype(np.float64)
    f32 = {k: np.ascontiguousarray(f[k], dtype=np.float32) for k in G.SWC_IN}
    # (the file holds float32: MAPL_UNDEF as the float32 the fields carry, so that the real(8) build recognises it too)
    consts = G.swc_consts(co2=f["CO2"], UNDEF=float(np.float32(G.MAPL["UNDEF"])))
    hk = np.concatenate([np.asarray(f["HK_UV"], dtype=np.float32).ravel(), np.asarray(f["HK_IR"], dtype=np.float32).ravel()])
    dark = {k: -100.0 - 0.5 * i for i, k in enumerate(G.SWC_OUT)}
    sentinel = -7.0
    fin, fout = tmp_path / "in.bin", tmp_path / "out.bin"
    with open(fin, "wb") as fh:
        np.array([ncol, lm, f["LCLDMH"], f["LCLDLM"]], dtype=np.int32).tofile(fh)
        np.array(consts, dtype=np.float64).tofile(fh)
        zth.tofile(fh)
        for k in G.SWC_IN:
            f32[k].tofile(fh)
        hk.tofile(fh)
        np.array([dark[k] for k in G.SWC_OUT] + [sentinel], dtype=np.float32).tofile(fh)
    env = dict(os.environ, GEOSRAD_DATA=os.path.join(ROOT, "geosradiation_gridcomp_amd", "data"))
    subprocess.check_call([exe, str(fin), str(fout)], env=env)
    raw = np.fromfile(fout, dtype=np.float64)
    n3p = (lm + 1) * ncol
    assert int(raw[0]) == int(day.sum())
    got = dict(zip(["FSW", "FSWU", "NIRR", "FSWBAND", "DRBAND"], np.split(raw[1:], np.cumsum([n3p, n3p, ncol, 8 * ncol]))))
    # the Python call
    ctx = gpu_ctx[4 if kind == "r4" else 8]
    dt = ctx.dtype
    tdt = torch.float32 if kind == "r4" else torch.float64
    st = torch.cuda.current_stream().cuda_stream
    t = {k: torch.from_numpy(v.astype(dt)).cuda() for k, v in f32.items()}
    for k in G.SWC_OUT:
        shp = (lm + 1, ncol) if k in ("FSW", "FSC", "FSWU", "FSCU") else ((8, ncol) if k in ("FSWBAND", "DRBAND", "DFBAND") else (ncol,))
        t[k] = torch.full(shp, sentinel, dtype=tdt, device="cuda")
    tz = torch.from_numpy(zth.astype(dt)).cuda()
    idx = torch.zeros(ncol, dtype=torch.int32, device="cuda"); pos = torch.zeros(ncol, dtype=torch.int32, device="cuda")
    nl = torch.zeros(1, dtype=torch.int32, device="cuda")
    nlit = ctx.lit_index_dev(st, ncol, tz.data_ptr(), idx.data_ptr(), pos.data_ptr(), nl.data_ptr())
    ctx.sw_driver_chou_lit_dev(st, ncol, nlit, idx.data_ptr(), pos.data_ptr(), lm, {k: v.data_ptr() for k, v in t.items()}, consts,
                               f["LCLDMH"], f["LCLDLM"], hk[:5], hk[5:], do_drfband=True, dark=dark, keep=("DRBAND",))
    ctx.check(st)
    for k, v in got.items():
        np.testing.assert_array_equal(v, t[k].cpu().numpy().astype(np.float64).ravel(), err_msg=k)
    fsw = got["FSW"].reshape(lm + 1, ncol)
    assert (fsw[0, day] > 0.3).all() and (fsw[:, ~day] == dark["FSW"]).all()
    drb = got["DRBAND"].reshape(8, ncol)
    assert (drb[:, ~day] == sentinel).all() and (drb[:, day] >= 0).all()
