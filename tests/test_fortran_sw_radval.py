"""GPU: the Fortran drop-in of a SOLAR_RADVAL build.  sw_radval_driver.F90 calls rrtmg_sw with the reference's long argument list
(SW/rrtmg_sw_rad.F90:68-124) against the shim modules compiled -DSOLAR_RADVAL; its 120 arrays must be the Python call's bit for bit, and
the outputs both flavours have must be those of sw_driver.F90 against the plain shim, bit for bit."""
import os
import subprocess

import numpy as np
import pytest

from tests import sw_radval_util as U
from tests.conftest import ROOT
from tests.test_fortran_shim import FDIR, SW_ORDER

pytestmark = pytest.mark.gpu


def _write(path, inp, ih, iaer, normFlx, isolvar, scon, iceflg=None):
    nlay, ncol = inp["play"].shape
    with open(path, "wb") as f:
        np.array([ncol, nlay, ih, int(inp["dyofyr"]), int(inp["cloudLM"]), int(inp["cloudMH"]), iaer, normFlx, isolvar], dtype=np.int32).tofile(f)
        np.array([scon], dtype=np.float32).tofile(f)
        if iceflg is not None:
            np.array([iceflg], dtype=np.int32).tofile(f)
        for k in SW_ORDER:
            np.ascontiguousarray(inp[k], dtype=np.float32).tofile(f)


def _read(path, nlay, ncol, radval):
    raw = np.fromfile(path, dtype=np.uint8)
    assert int(raw[:4].view(np.int32)[0]) == 0
    raw = raw[4:]
    off = 0

    def take(shape):
        nonlocal off
        n = int(np.prod(shape))
        a = raw[off: off + n * 8].view(np.float64).reshape(shape); off += n * 8
        return a
    got = {k: take((nlay + 1, ncol)) for k in ("swuflx", "swdflx", "swuflxc", "swdflxc")}
    got["nirr"] = take((ncol,)); got["parf"] = take((ncol,))
    for k in ("fswband", "drband", "dfband"):
        got[k] = take((14, ncol))
    got["cotdtp"] = take((ncol,))
    if radval:
        for k in ("cotdhp", "cotdmp", "cotdlp", "cotntp", "cotnhp", "cotnmp", "cotnlp"):
            got[k] = take((ncol,))
        got["radval"] = take((120, ncol))
    got["clearCounts"] = raw[off:].view(np.int32).reshape(4, ncol)
    return got


@pytest.mark.parametrize("kind", ["r8", "r4"])
def test_fortran_solar_radval_caller(tmp_path, kind):
    from geosradiation_gridcomp_amd import synth
    from geosradiation_gridcomp_amd.api import Context, RADVAL_NAMES
    exe = os.path.join(FDIR, "bin", f"sw_radval_driver_{kind}")
    plain = os.path.join(FDIR, "bin", f"sw_driver_{kind}")
    if not (os.path.exists(exe) and os.path.exists(plain)):
        subprocess.check_call(["make", "-s", "-C", FDIR])
    ncol, nlay, ih = 75, 72, 1
    inp = U.both_phases(synth.make_columns(ncol, nlay, start=808, aerosol=True, cloudy_frac=0.6))
    # the callers read fp32 files: both sides start from the same fp32 values
    inp = {k: (np.asarray(v, dtype=np.float32) if isinstance(v, np.ndarray) and v.dtype.kind == "f" else v) for k, v in inp.items()}
    env = dict(os.environ, GEOSRAD_DATA=os.path.join(ROOT, "geosradiation_gridcomp_amd", "data"))
    fin, fout = tmp_path / "in.bin", tmp_path / "out.bin"
    _write(fin, inp, ih, 10, 1, 0, 1361.0, iceflg=3)
    subprocess.check_call([exe, str(fin), str(fout)], env=env)
    f = _read(fout, nlay, ncol, True)
    ctx = Context(8 if kind == "r8" else 4)
    try:
        ctx.set_inhomogeneity(ih)
        g = ctx.rrtmg_sw_columns(inp, iaer=10, normFlx=1, do_drfband=True, radval=True)
    finally:
        ctx.close()
    assert (g["radval"] != 0).any(axis=1).all()
    for k, name in enumerate(RADVAL_NAMES):
        np.testing.assert_array_equal(f["radval"][k], g[name].astype(np.float64), err_msg=name)
    for k in ("swuflx", "swdflx", "swuflxc", "swdflxc", "nirr", "parf", "fswband", "drband", "dfband", "cotdtp", "cotnlp"):
        np.testing.assert_array_equal(f[k], g[k].astype(np.float64), err_msg=k)
    np.testing.assert_array_equal(f["clearCounts"], g["clearCounts"])
    # the plain flavour (sw_driver: iceflgsw 3, the short argument list) on the same batch: what both have is the same bits
    fin2, fout2 = tmp_path / "in2.bin", tmp_path / "out2.bin"
    _write(fin2, inp, ih, 10, 1, 0, 1361.0)
    subprocess.check_call([plain, str(fin2), str(fout2)], env=env)
    p = _read(fout2, nlay, ncol, False)
    for k, v in p.items():
        np.testing.assert_array_equal(v, f[k], err_msg=k)
