"""Heartbeat McICA cloud fractions of the Solar GridComp's UPDATE_EXPORT on the device (geosrad_sw_update_cldhb_dev /
Context.sw_update_cldhb_dev): CLDTTSWHB, CLDHISWHB, CLDMDSWHB, CLDLOSWHB of GEOS_SolarGridComp.F90:7060-7223 (SOLAR_RADVAL).

The yardstick is tests/sw_cldhb_util.py: a numpy restatement of the block's preparation, then a generator + clearCounts_threeBand.  On
the CPU the restatement's arrays give the same counts through the reference's own Fortran (oracle/reflib.py) and through the oracle
(oracle/clib.py), in the vertical ordering only this call site uses (TOA first).  On the GPU the fp64 exports equal the oracle's
bitwise; the fp32 exports equal, bitwise, the composition of the device's existing generate_stochastic_clouds_dev and
clearCounts_threeBand on the restatement's float32 arrays (entry points that carry the project's fp32 bound against the reference);
how many fp32 columns differ from the r4 oracle is printed, not asserted."""
import os
import subprocess

import numpy as np
import pytest

from tests.conftest import ROOT
from tests import sw_cldhb_util as U
from oracle import reflib

SHAPES = [(130, 72, 41), (70, 37, 43)]      # (ncol, lm, seed): two full waves + two lanes, clear and cloudy columns mixed in a wave
DOYS = [45, 250]                            # either side of day 181 (correlation_length's two branches)
KIND = {4: "r4", 8: "r8"}


# ---- CPU -----------------------------------------------------------------------------------------------------------------------------
def test_symbol_exported():
    from geosradiation_gridcomp_amd import _lib
    assert "geosrad_sw_update_cldhb_dev" in _lib.EXPORTS
    L = _lib.lib()
    assert hasattr(L, "geosrad_sw_update_cldhb_dev")
    assert L.geosrad_sw_update_cldhb_dev(None, None, 1, 10, 4, 7, 100, None, None, None) == 1     # EINVAL, null context


def test_header_orders_match_gridcomp_lists():
    import re
    from geosradiation_gridcomp_amd import gridcomp as G
    h = open(os.path.join(ROOT, "include", "geosrad.h")).read()
    enums = [re.findall(r"GEOSRAD_SWHB_(\w+)", e) for e in re.findall(r"enum\s*\{([^}]*GEOSRAD_SWHB_[^}]*)\}", h)]
    assert len(enums) == 3
    ins, consts, outs = enums
    assert ins[-1] == "NIN" and ins[:-1] == G.SWHB_IN
    assert consts[-1] == "NCONST" and [c[2:] for c in consts[:-1]] == G.SWHB_CONST
    assert outs[-1] == "NOUT" and outs[:-1] == G.SWHB_OUT == U.OUT
    assert G.swhb_consts() == [U.GRAV, U.RGAS]
    F = open(os.path.join(ROOT, "geosradiation_gridcomp_amd", "fortran", "gridcomp_shims.F90")).read()
    for names in (G.SWHB_IN, G.SWHB_OUT):
        for i, k in enumerate(names):
            assert re.search(rf"\bSWHB_{k}\s*=\s*{i + 1}\b", F), k


@pytest.mark.skipif(not reflib.available("r4"), reason="oracle/_ref not built (needs /root/reference + flang)")
@pytest.mark.parametrize("ih", [0, 1, 2])
@pytest.mark.parametrize("kind", ["r4", "r8"])
def test_restatement_counts_reference_equals_oracle(kind, ih):
    """the restatement's TOA-first arrays through the reference's generate_stochastic_clouds + clearCounts_threeBand and through the
    oracle's: the same counts, so the oracle is pinned to the reference in this call site's ordering and seeding"""
    from oracle import clib
    dt = reflib.dtype_of(kind)
    f, mh, ml = U.make_fields(40, 72, seed=7)
    p = U.prepare(f, dt)
    cols = U.cloudy_columns(f)
    assert 10 < len(cols) < 40 and (p["play"][0] < p["play"][-1]).all()
    reflib.set_inhomogeneity(ih, kind); clib.set_inhomogeneity(ih, kind)
    try:
        a = U.clear_counts(p, cols, 200, mh, ml, "reflib", kind=kind)
        b = U.clear_counts(p, cols, 200, mh, ml, "clib", kind=kind)
    finally:
        reflib.set_inhomogeneity(0, kind); clib.set_inhomogeneity(0, kind)
    np.testing.assert_array_equal(a, b)
    assert (a[:, 0] < U.NSUB).any() and (a[:, 0] > 0).any() and (a[:, 1:] < U.NSUB).any(axis=0).all()


def test_cfac_constant_in_float32():
    """cfac = 1.02 * 100 * dp (:7138): the constant is formed first, in the real kind; in float32 it is 102 exactly"""
    assert np.float32(1.02) * np.float32(100) == np.float32(102.0) and np.float64(1.02) * np.float64(100) == 102.0


# ---- GPU -----------------------------------------------------------------------------------------------------------------------------
def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def _run(ctx, f, mh, ml, doy, names=None, sentinel=-7.0, drop=(), consts=None, ncol=None, lm=None):
    """the device entry point on fields f; exports `names` (default all four), the others allocated, sentinel-filled, not passed"""
    import torch
    from geosradiation_gridcomp_amd import gridcomp as G
    dt = ctx.dtype
    flm, fncol = f["FCLD"].shape
    t = {k: torch.from_numpy(np.ascontiguousarray(f[k], dtype=dt)).cuda() for k in G.SWHB_IN if k not in drop}
    tdt = torch.float32 if dt == np.float32 else torch.float64
    o = {k: torch.full((fncol,), sentinel, dtype=tdt, device="cuda") for k in G.SWHB_OUT}
    ptr = {k: v.data_ptr() for k, v in t.items()}
    ptr.update({k: o[k].data_ptr() for k in (G.SWHB_OUT if names is None else names)})
    try:
        ctx.sw_update_cldhb_dev(_stream(), fncol if ncol is None else ncol, flm if lm is None else lm, mh, ml, doy, ptr, consts=consts)
        ctx.check(_stream())
    finally:
        torch.cuda.synchronize()
    return np.stack([o[k].cpu().numpy() for k in G.SWHB_OUT])


_BATCH = {}


def _batch(gpu_ctx, rk, ih):
    """the parity batch of one (real kind, inhomogeneity): per (shape, doy) the fields, the device's exports and the yardstick's;
    computed once, shared by the tests below, left unchanged"""
    if (rk, ih) not in _BATCH:
        from oracle import clib
        ctx = gpu_ctx[rk]; dt = ctx.dtype
        ctx.set_inhomogeneity(ih); clib.set_inhomogeneity(ih, KIND[rk])
        try:
            runs = []
            for ncol, lm, seed in SHAPES:
                f, mh, ml = U.make_fields(ncol, lm, seed=seed)
                p = U.prepare(f, dt)
                for doy in DOYS:
                    got = _run(ctx, f, mh, ml, doy)
                    ora, ocnt = U.exports(f, dt, doy, mh, ml, "clib", kind=KIND[rk], p=p)
                    dev = U.exports(f, dt, doy, mh, ml, "device", ctx=ctx, p=p)[0] if rk == 4 else None
                    runs.append(dict(f=f, mh=mh, ml=ml, doy=doy, got=got, oracle=ora, oracle_cnt=ocnt, device=dev))
        finally:
            ctx.set_inhomogeneity(0); clib.set_inhomogeneity(0, KIND[rk])
        _BATCH[(rk, ih)] = runs
    return _BATCH[(rk, ih)]


@pytest.mark.gpu
@pytest.mark.parametrize("ih", [0, 1, 2])
@pytest.mark.parametrize("rk", [4, 8])
def test_exports_match_the_reference_path(gpu_ctx, rk, ih, capsys):
    """130 x 72 and 70 x 37, two days of the year, latitudes in both hemispheres.  fp64: the oracle's 1 - count / 112, bitwise.
    fp32: the composition of the device's generator and clearCounts on the restatement's float32 arrays, bitwise; the number of columns
    whose counts differ from the r4 oracle's is printed."""
    for r in _batch(gpu_ctx, rk, ih):
        f = r["f"]
        mixed = (f["FCLD"] > 0).any(axis=0)[:64]
        assert mixed.any() and not mixed.all() and (f["LATS"] > 0).any() and (f["LATS"] < 0).any()
        want = r["oracle"] if rk == 8 else r["device"]
        np.testing.assert_array_equal(r["got"], want, err_msg=f"r{rk} ih {ih} {f['FCLD'].shape} doy {r['doy']}")
        part = (r["oracle_cnt"] > 0) & (r["oracle_cnt"] < U.NSUB)
        assert part.any(axis=1).all()                  # every export has partly cloudy columns in the batch
        if rk == 4:
            ndiff = int((r["got"] != r["oracle"]).any(axis=0).sum())
            with capsys.disabled():
                print(f"sw_update_cldhb fp32, ih {ih}, {f['FCLD'].shape[1]} x {f['FCLD'].shape[0]}, doy {r['doy']}: columns whose counts differ "
                      f"from the r4 oracle's: {ndiff} of {int((f['FCLD'] > 0).any(axis=0).sum())} cloudy")


def _hand(lm, mh, ml, dt):
    """columns whose only cloud is one layer with FCLD = 1 and QL > 0, at layers 1, mh-1, mh, ml-1, ml, lm (in this order); then a
    column with cloud fraction but no condensate; then a column without cloud fraction (but condensate)"""
    base, _, _ = U.make_fields(8, lm, seed=3)
    layers = [1, mh - 1, mh, ml - 1, ml, lm]
    f = {k: (v.copy()) for k, v in base.items()}
    f["FCLD"][:] = 0.0; f["QI"][:] = 0.0; f["QL"][:] = 0.0
    for i, l in enumerate(layers):
        f["FCLD"][l - 1, i] = 1.0; f["QL"][l - 1, i] = 1.0e-4
    f["FCLD"][lm // 2:, 6] = 0.7
    f["QL"][:, 7] = 1.0e-4; f["QI"][:, 7] = 1.0e-5
    return {k: v.astype(dt) for k, v in f.items()}, layers


@pytest.mark.gpu
@pytest.mark.parametrize("rk", [4, 8])
def test_single_layer_clouds_land_in_their_super_layer(gpu_ctx, rk):
    """deterministic, no reference: an overcast layer with condensate makes its super-layer and the column exactly 1 and the other two
    exactly 0, at every super-layer boundary; no condensate (the cwp_tiny reset) and no cloud fraction give exactly 0; lm = 4 runs"""
    ctx = gpu_ctx[rk]
    for lm, mh, ml in ((72, U.make_fields(1, 72, 0)[1], U.make_fields(1, 72, 0)[2]), (4, 2, 3)):
        f, layers = _hand(lm, mh, ml, ctx.dtype)
        got = _run(ctx, f, mh, ml, 100)
        for i, l in enumerate(layers):
            band = 1 if l < mh else (2 if l < ml else 3)
            want = [1.0] + [1.0 if b == band else 0.0 for b in (1, 2, 3)]
            assert got[:, i].tolist() == want, (lm, l, got[:, i])
        assert (got[:, 6] == 0).all() and (got[:, 7] == 0).all()


@pytest.mark.gpu
@pytest.mark.parametrize("rk", [4, 8])
def test_invariants_of_the_exports(gpu_ctx, rk):
    for ih in (0, 1, 2):
        for r in _batch(gpu_ctx, rk, ih):
            g = r["got"].astype(np.float64)
            cld = np.rint(g * U.NSUB)                                     # cloudy sub-columns
            assert (g >= 0).all() and (g <= 1).all()
            dt = r["got"].dtype.type
            np.testing.assert_array_equal(r["got"], dt(1.) - (U.NSUB - cld).astype(dt) / dt(U.NSUB))      # multiples of 1/112
            assert (cld[0] >= cld[1:].max(axis=0)).all()                  # CLDTT >= max(HI, MD, LO)
            assert (cld[0] <= cld[1:].sum(axis=0)).all()                  # a cloudy sub-column is cloudy in some super-layer
            clear = ~(r["f"]["FCLD"] > 0).any(axis=0)
            assert clear.any() and (r["got"][:, clear] == 0).all()


@pytest.mark.gpu
@pytest.mark.parametrize("rk", [4, 8])
def test_a_column_gives_the_same_bits_wherever_it_stands(gpu_ctx, rk):
    """seeds are per column: a cloudy column alone, first and last of the 130, and under ragged chunks (64 + 64 + 2)"""
    ctx = gpu_ctx[rk]
    r = _batch(gpu_ctx, rk, 1)[0]
    ctx.set_inhomogeneity(1)
    try:
        f, mh, ml, doy = r["f"], r["mh"], r["ml"], r["doy"]
        n = f["FCLD"].shape[1]
        part = np.flatnonzero((r["got"][0] > 0) & (r["got"][0] < 1))
        j = int(part[len(part) // 2])
        one = {k: np.ascontiguousarray(v[..., j:j + 1]) for k, v in f.items()}
        np.testing.assert_array_equal(_run(ctx, one, mh, ml, doy)[:, 0], r["got"][:, j])
        for pos in (0, n - 1):
            order = np.arange(n); order[pos], order[j] = j, pos
            g = _run(ctx, {k: np.ascontiguousarray(v[..., order]) for k, v in f.items()}, mh, ml, doy)
            np.testing.assert_array_equal(g[:, pos], r["got"][:, j])
            np.testing.assert_array_equal(g, r["got"][:, order])
        ctx.set_chunk(64)
        try:
            np.testing.assert_array_equal(_run(ctx, f, mh, ml, doy), r["got"])
        finally:
            ctx.set_chunk(131072)
    finally:
        ctx.set_inhomogeneity(0)


@pytest.mark.gpu
@pytest.mark.parametrize("rk", [4, 8])
def test_outputs_and_errors(gpu_ctx, rk):
    from geosradiation_gridcomp_amd import gridcomp as G
    from geosradiation_gridcomp_amd.api import Context, GeosradError
    ctx = gpu_ctx[rk]
    r = _batch(gpu_ctx, rk, 0)[0]
    f, mh, ml, doy = r["f"], r["mh"], r["ml"], r["doy"]
    lm = f["FCLD"].shape[0]
    # one export alone: the same bits, the other three untouched; none at all: OK, nothing written (inputs are then not looked at)
    o = _run(ctx, f, mh, ml, doy, names=["CLDMD"], sentinel=-3.0)
    np.testing.assert_array_equal(o[2], r["got"][2])
    assert (o[[0, 1, 3]] == -3.0).all()
    assert (_run(ctx, f, mh, ml, doy, names=[], sentinel=-3.0) == -3.0).all()
    assert (_run(ctx, f, mh, ml, doy, names=[], sentinel=-3.0, drop=tuple(G.SWHB_IN)) == -3.0).all()
    # the consts default to MAPL's values
    np.testing.assert_array_equal(_run(ctx, f, mh, ml, doy, consts=[U.GRAV, U.RGAS]), r["got"])
    # EINVAL, nothing written
    bad = [dict(mh=1), dict(mh=ml), dict(ml=lm + 1), dict(mh=ml, ml=mh), dict(ncol=0), dict(ncol=-3), dict(lm=3, mh=2, ml=3)]
    bad += [dict(drop=(k,)) for k in G.SWHB_IN] + [dict(drop=("QL",), names=["CLDLO"])]
    for b in bad:
        with pytest.raises(GeosradError):
            _run_keep(ctx, f, b.get("mh", mh), b.get("ml", ml), doy, b)
    # a context without solver or inhomogeneity tables, ih = 0: the same bits; a multi-device context answers like every `_dev` entry
    bare = Context(rk, tables=False)
    try:
        np.testing.assert_array_equal(_run(bare, f, mh, ml, doy), r["got"])
    finally:
        bare.close()
    multi = Context(rk, tables=False, devices=[0, 0])
    try:
        with pytest.raises(GeosradError, match="single-device"):
            _run(multi, f, mh, ml, doy)
    finally:
        multi.close()


def _run_keep(ctx, f, mh, ml, doy, b):
    """_run for a call that must fail with sentinels untouched: the check runs whether or not the call raises"""
    import torch
    from geosradiation_gridcomp_amd import gridcomp as G
    dt = ctx.dtype
    lm, ncol = f["FCLD"].shape
    tdt = torch.float32 if dt == np.float32 else torch.float64
    t = {k: torch.from_numpy(np.ascontiguousarray(f[k], dtype=dt)).cuda() for k in G.SWHB_IN if k not in b.get("drop", ())}
    o = {k: torch.full((ncol,), -5.0, dtype=tdt, device="cuda") for k in G.SWHB_OUT}
    ptr = {k: v.data_ptr() for k, v in t.items()}
    ptr.update({k: o[k].data_ptr() for k in b.get("names", G.SWHB_OUT)})
    try:
        ctx.sw_update_cldhb_dev(_stream(), b.get("ncol", ncol), b.get("lm", lm), mh, ml, doy, ptr)
    finally:
        torch.cuda.synchronize()
        for k, v in o.items():
            assert (v == -5.0).all().item(), (b, k)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["r8", "r4"])
def test_fortran_caller_equals_c_entry_point(tmp_path, gpu_ctx, kind):
    """swcldhb_driver.F90: set_inhomogeneity(1) and `call sw_update_cldhb` (module geosrad_gridcomp) on device fields give the C entry
    point's bits"""
    from geosradiation_gridcomp_amd import gridcomp as G
    fdir = os.path.join(ROOT, "geosradiation_gridcomp_amd", "fortran")
    exe = os.path.join(fdir, "bin", f"swcldhb_driver_{kind}")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-s", "-C", fdir])
    rk = 4 if kind == "r4" else 8
    ctx = gpu_ctx[rk]; dt = ctx.dtype
    ncol, lm, seed = SHAPES[0]
    f, mh, ml = U.make_fields(ncol, lm, seed=seed)
    f32 = {k: np.ascontiguousarray(f[k], dtype=np.float32) for k in G.SWHB_IN}
    doy, ih = 250, 1
    fin, fout = tmp_path / "in.bin", tmp_path / "out.bin"
    with open(fin, "wb") as fh:
        np.array([ncol, lm, mh, ml, doy, ih], dtype=np.int32).tofile(fh)
        for k in G.SWHB_IN:
            f32[k].tofile(fh)
    env = dict(os.environ, GEOSRAD_DATA=os.path.join(ROOT, "geosradiation_gridcomp_amd", "data"))
    subprocess.check_call([exe, str(fin), str(fout)], env=env)
    got = np.fromfile(fout, dtype=np.float64).reshape(4, ncol)
    # the Fortran caller passes MAPL_GRAV and MAPL_RGAS = MAPL_RUNIV / MAPL_AIRMW as constants of its real kind
    consts = [float(dt(9.80665)), float(dt(8314.47) / dt(28.965))]
    ctx.set_inhomogeneity(ih)
    try:
        want = _run(ctx, f32, mh, ml, doy, consts=consts)
    finally:
        ctx.set_inhomogeneity(0)
    np.testing.assert_array_equal(got, want.astype(np.float64))
    assert ((want[0] > 0) & (want[0] < 1)).any()
