"""SOLAR_RADVAL diagnostics of rrtmg_sw on the GPU (Context.rrtmg_sw_radval / rrtmg_sw_radval_dev / rrtmg_sw_columns(radval=True)):
the reference's dummy arguments cdsdtp .. forinlp (SW/rrtmg_sw_rad.F90:86-119) against the plain-C restatement tests/sw_radval_impl.h.

The reference's argument list has 15 families x {d, n} x {tp, hp, mp, lp} = 120 arrays (30 lines of four names, :86-119).

Bound: the one tests/test_gpu_sw.py uses for the cotd?? / cotn?? family, 1e-11 (fp64) / 2e-5 (fp32) of max(|ref|, 1), on the columns
selected as there: in fp64 clearCounts must equal the restatement's and no column is left out; in fp32 the columns whose clearCounts
differ (a sub-column decision flipped by the fp32 exp of the overlap correlation) are left out, at most 5 % of the batch."""
import os

import numpy as np
import pytest

from tests import sw_radval_util as U

pytestmark = pytest.mark.gpu

KEYS = ("swuflx", "swdflx", "swuflxc", "swdflxc", "nirr", "nirf", "parr", "parf", "uvrr", "uvrf", "fswband", "clearCounts",
        "cotdtp", "cotdhp", "cotdmp", "cotdlp", "cotntp", "cotnhp", "cotnmp", "cotnlp")
# (iceflg, isolvar, nlay, ncol): every iceflg with every isolvar at 72 layers, two 137-layer cases; the column counts are ragged
CASES = [(ice, iso, 72, 203) for ice in (1, 2, 3, 4) for iso in (-1, 0, 2)] + [(3, 0, 137, 131), (2, -1, 137, 131), (4, 2, 137, 131)]


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return U.build_ref(tmp_path_factory.mktemp("sw_radval"))


@pytest.fixture(scope="module")
def ctxs():
    """contexts per (real_kind, GEOSRAD_SW_PATH): the path is read when the context is created"""
    from geosradiation_gridcomp_amd.api import Context
    made = {}
    old = os.environ.get("GEOSRAD_SW_PATH")
    try:
        for path in ("reform", "bands"):
            if path == "bands":
                os.environ["GEOSRAD_SW_PATH"] = "bands"
            else:
                os.environ.pop("GEOSRAD_SW_PATH", None)
            for rk in (8, 4):
                made[(rk, path)] = Context(rk)
    finally:
        if old is None:
            os.environ.pop("GEOSRAD_SW_PATH", None)
        else:
            os.environ["GEOSRAD_SW_PATH"] = old
    yield made
    for c in made.values():
        c.close()


def _batch(nlay, ncol, start):
    from geosradiation_gridcomp_amd import synth
    return U.both_phases(synth.make_columns(ncol, nlay, start=start, aerosol=True, cloudy_frac=0.6))


def test_paths_are_the_two_band_sweeps(ctxs):
    from geosradiation_gridcomp_amd import _lib
    L = _lib.lib()
    assert L.geosrad_kernel_label(ctxs[(4, "reform")].h, 8) == b"k_sw_reform" and L.geosrad_kernel_label(ctxs[(4, "bands")].h, 8) == b"k_sw_bands"


@pytest.mark.parametrize("case", range(len(CASES)))
@pytest.mark.parametrize("path", ["reform", "bands"])
@pytest.mark.parametrize("rk", [8, 4])
def test_radval_matches_restatement(ctxs, ref, rk, path, case):
    from geosradiation_gridcomp_amd.api import RADVAL_NAMES
    ice, iso, nlay, ncol = CASES[case]
    kind = "r8" if rk == 8 else "r4"
    inp = _batch(nlay, ncol, 7000 + 37 * case)
    o = ref.radval(inp, kind, isolvar=iso, iceflg=ice)
    assert o["rc"] == 0
    U.assert_coverage(o["radval"], inp, RADVAL_NAMES)          # the inputs exercise every one of the 120 outputs
    ctx = ctxs[(rk, path)]
    g = ctx.rrtmg_sw_columns(inp, isolvar=iso, iceflg=ice, iaer=10 if case % 2 else 0, normFlx=case % 3 == 0, radval=True)
    if rk == 8:
        np.testing.assert_array_equal(g["clearCounts"], o["clearCounts"])
        same = np.ones(ncol, dtype=bool)
    else:
        same = (g["clearCounts"] == o["clearCounts"]).all(axis=0)
        assert same.mean() >= 0.95
    want = o["radval"].astype(np.float64)
    got = g["radval"].astype(np.float64)
    err = np.abs(got - want) / np.maximum(np.abs(want), 1.0)
    worst = err[:, same].max(axis=1)
    k = int(worst.argmax())
    print(f"radval rk={rk} path={path} case={CASES[case]}: worst relative error {worst[k]:.3e} in {RADVAL_NAMES[k]}; "
          f"{int((~same).sum())} of {ncol} columns left out")
    assert worst[k] <= (1e-11 if rk == 8 else 2e-5), (RADVAL_NAMES[k], worst[k])
    for j, name in enumerate(RADVAL_NAMES):
        assert g[name] is not None and np.array_equal(g[name], g["radval"][j])
    # cloud-free columns: zeros (rrtmg_sw_rad.F90:1540)
    assert (g["radval"][:, ~U.cloudy_columns(inp)] == 0).all()


@pytest.mark.parametrize("path", ["reform", "bands"])
@pytest.mark.parametrize("rk", [8, 4])
def test_existing_outputs_unchanged_and_identities(ctxs, rk, path):
    """The outputs rrtmg_sw already had are the same bits with and without the diagnostics; and the identities that hold bit for bit
    because the reference accumulates the same product under the same guard (SW/rrtmg_sw_spcvmc.F90:799-825)."""
    from geosradiation_gridcomp_amd.api import RADVAL_NAMES
    ctx = ctxs[(rk, path)]
    inp = _batch(72, 211, 4321)
    for kw in (dict(iaer=10, do_drfband=True), dict(iaer=0, normFlx=1, isolvar=2, iceflg=2)):
        a = ctx.rrtmg_sw_columns(inp, **kw)
        b = ctx.rrtmg_sw_columns(inp, radval=True, **kw)
        for k in KEYS + (("drband", "dfband") if kw.get("do_drfband") else ()):
            np.testing.assert_array_equal(a[k], b[k], err_msg=k)
        for p in "li":
            for sl in ("tp", "hp", "mp", "lp"):
                eq = lambda x, y: np.testing.assert_array_equal(b[x + sl], b[y + sl], err_msg=f"{x}{sl} {y}{sl}")
                eq(f"ssa{p}d", f"cot{p}n"); eq(f"asm{p}d", f"ssa{p}n"); eq(f"sds{p}d", f"cds{p}n")
                eq(f"for{p}d", f"ads{p}d"); eq(f"ads{p}d", f"sds{p}n")
        assert len(RADVAL_NAMES) == b["radval"].shape[0]


@pytest.mark.parametrize("path", ["reform", "bands"])
@pytest.mark.parametrize("rk", [8, 4])
def test_liquid_only_and_cloud_free_columns(ctxs, rk, path):
    from geosradiation_gridcomp_amd import synth
    from tests.conftest import sub_columns
    ctx = ctxs[(rk, path)]
    inp = synth.make_columns(512, 72, start=77, cloudy_frac=0.6)          # unaltered: liquid in warm decks, ice in cold ones
    cld = np.asarray(inp["cldf"]) > 0
    liq_only = cld.any(axis=0) & ~((np.asarray(inp["ciwp"]) > 0) & cld).any(axis=0)
    clear = ~cld.any(axis=0)
    assert liq_only.sum() >= 20 and clear.sum() >= 20
    g = ctx.rrtmg_sw_columns(inp, radval=True)
    assert (g["radval"][:, clear] == 0).all()
    for sl in ("tp", "hp", "mp", "lp"):
        for dn in "dn":
            for f in ("coti", "cdsi", "ssai", "sdsi", "asmi", "adsi", "fori"):
                assert (g[f + dn + sl][liq_only] == 0).all(), f + dn + sl
            np.testing.assert_array_equal(g["cotl" + dn + sl][liq_only], g["cot" + dn + sl][liq_only])
            np.testing.assert_array_equal(g["cdsl" + dn + sl][liq_only], g["cds" + dn + sl][liq_only])
    assert (g["cotlntp"][liq_only] > 0).any()


@pytest.mark.parametrize("rk", [8, 4])
def test_host_entry_equals_dev_entry_across_chunks(ctxs, rk):
    import torch
    ctx = ctxs[(rk, "reform")]
    inp = _batch(72, 301, 999)
    nlay, ncol = inp["play"].shape
    ctx.set_chunk(128)                                          # splits the batch into three chunks, the last one ragged
    try:
        h = ctx.rrtmg_sw_columns(inp, iaer=10, radval=True)
    finally:
        ctx.set_chunk(131072)
    dt = torch.float64 if rk == 8 else torch.float32
    names = ["coszen", "play", "plev", "tlay", "h2ovmr", "o3vmr", "co2vmr", "ch4vmr", "o2vmr", "cldf", "ciwp", "clwp", "rei", "rel", "zm",
             "alat", "tauaer_sw", "ssaaer_sw", "asmaer_sw", "asdir", "asdif", "aldir", "aldif"]
    t = {k: torch.from_numpy(np.ascontiguousarray(inp[k], dtype=ctx.dtype)).cuda() for k in names}
    for k in ("swuflx", "swdflx", "swuflxc", "swdflxc"):
        t[k] = torch.zeros((nlay + 1, ncol), dtype=dt, device="cuda")
    for k in ("nirr", "nirf", "parr", "parf", "uvrr", "uvrf") + KEYS[12:]:
        t[k] = torch.zeros(ncol, dtype=dt, device="cuda")
    t["fswband"] = torch.zeros((14, ncol), dtype=dt, device="cuda")
    t["clearCounts_sw"] = torch.zeros((4, ncol), dtype=torch.int32, device="cuda")
    t["radval"] = torch.full((120, ncol), -1.0, dtype=dt, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    ptr = {k: v.data_ptr() for k, v in t.items()}
    ctx.rrtmg_sw_radval_dev(stream, ncol, nlay, 1361.0, 1.0, 0, ptr, 3, 1, inp["dyofyr"], 10, inp["cloudLM"], inp["cloudMH"])
    ctx.check(stream)
    np.testing.assert_array_equal(t["radval"].cpu().numpy(), h["radval"])
    np.testing.assert_array_equal(t["clearCounts_sw"].cpu().numpy(), h["clearCounts"])
    for k in ("swuflx", "fswband", "cotntp"):
        np.testing.assert_array_equal(t[k].cpu().numpy(), h[k], err_msg=k)
    # the plain device entry point on the same inputs: the outputs it has are the same bits
    t2 = {k: (torch.zeros_like(v) if k in ("swuflx", "swdflx", "swuflxc", "swdflxc", "fswband", "clearCounts_sw") or v.shape == (ncol,) and k not in names else v)
          for k, v in t.items()}
    ptr2 = {k: v.data_ptr() for k, v in t2.items()}
    ctx.rrtmg_sw_dev(stream, ncol, nlay, 1361.0, 1.0, 0, ptr2, 3, 1, inp["dyofyr"], 10, inp["cloudLM"], inp["cloudMH"])
    ctx.check(stream)
    for k in ("swuflx", "swdflx", "swuflxc", "swdflxc", "fswband", "clearCounts_sw", "nirr", "parf") + KEYS[12:]:
        np.testing.assert_array_equal(t2[k].cpu().numpy(), t[k].cpu().numpy(), err_msg=k)


def test_workspace_is_taken_only_when_requested():
    from geosradiation_gridcomp_amd import synth
    from geosradiation_gridcomp_amd.api import Context
    inp = synth.make_columns(256, 72, start=5, cloudy_frac=0.5)
    ctx = Context(4)
    try:
        ctx.rrtmg_sw_columns(inp)
        w0 = ctx.workspace_bytes()
        ctx.rrtmg_sw_columns(inp)
        assert ctx.workspace_bytes() == w0
        ctx.rrtmg_sw_columns(inp, radval=True)
        w1 = ctx.workspace_bytes()
        assert 3 * 15 * 20 * 256 * 4 <= w1 - w0 <= 3 * 15 * 20 * 256 * 4 + 4096
    finally:
        ctx.close()


def test_multi_device_context_shards_radval():
    import torch
    if torch.cuda.device_count() < 2:
        pytest.skip("one device visible: geosrad_create_multi needs two")
    from geosradiation_gridcomp_amd.api import Context
    inp = _batch(72, 203, 31)
    one = Context(4)
    two = Context(4, devices=[0, 1])
    try:
        a = one.rrtmg_sw_columns(inp, radval=True); b = two.rrtmg_sw_columns(inp, radval=True)
        np.testing.assert_array_equal(a["radval"], b["radval"])
    finally:
        one.close(); two.close()
