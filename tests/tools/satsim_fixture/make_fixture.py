"""Regenerates tests/golden/satsim_isccp_72.npz from a checkout of the reference:

    python tests/tools/satsim_fixture/make_fixture.py --ref <GEOSsatsim_GridComp directory> [--work DIR] [--out FILE]

Compiles the reference's scops.f and icarus.f unmodified, in place, in r4 and r8 (flang -c -O1 -ffp-contract=off -I<ref>; r8 adds
-fdefault-real-8) with driver.f90 beside them in a work directory, runs both builds on satsim_util.make_batch(), checks what the issue
checked (identical masks and seeds, no sub-column moved between the two builds, the numpy restatement bit for bit on masks, seeds and
histogram) and stores inputs, outputs, the reference's own r4-against-r8 spread per continuous output (spread_*) and what the float64
restatement differs from the r8 build (restate64_*, restate64rel_*).  Nothing of the reference is copied into the repository."""
import argparse
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(HERE))))
from tests import satsim_util as U  # noqa: E402

NP, NL, NC = 96, 72, 30
SHAPES = dict(fq_isccp=(7, 7, NP), totalcldarea=(NP,), meanptop=(NP,), meantaucld=(NP,), meanalbedocld=(NP,), meantb=(NP,), meantbclr=(NP,),
              boxtau=(NC, NP), boxptop=(NC, NP))


def build(ref, work, kind, fc):
    d = os.path.join(work, kind)
    os.makedirs(d, exist_ok=True)
    flags = ["-O1", "-ffp-contract=off"] + (["-fdefault-real-8"] if kind == "r8" else [])
    for f in ("scops", "icarus"):
        subprocess.check_call([fc, "-c", *flags, "-I" + ref, os.path.join(ref, f + ".f"), "-o", os.path.join(d, f + ".o")])
    subprocess.check_call([fc, *flags, os.path.join(HERE, "driver.f90"), os.path.join(d, "scops.o"), os.path.join(d, "icarus.o"), "-o", os.path.join(d, "driver")])
    return d


def run(d, kind, b):
    dt = np.float32 if kind == "r4" else np.float64
    with open(os.path.join(d, "in.bin"), "wb") as f:
        np.array([NP, NL, NC], np.int32).tofile(f)
        b["sunlit"].astype(np.int32).tofile(f); b["seed"].astype(np.int32).tofile(f)
        for n in U.IN_2D:
            b[n].astype(dt).tofile(f)
        b["skt"].astype(dt).tofile(f); np.array([U.EMSFC_LW], dt).tofile(f)
    subprocess.check_call([os.path.join(d, "driver")], cwd=d)
    raw = open(os.path.join(d, "out.bin"), "rb")
    rd = lambda shape, t=dt: np.fromfile(raw, t, int(np.prod(shape))).reshape(shape)
    o = {}
    for ov in (1, 2, 3):
        fr = rd((NL, NC, NP))
        assert set(np.unique(fr)) <= {0., 1., 2.}
        o[f"mask_ov{ov}"] = fr.astype(np.uint8); o[f"seed_ov{ov}"] = rd((NP,), np.int32)
    for th, thd in U.OPTION_PAIRS:
        for n in U.ICARUS_OUT:
            o[f"{n}_th{th}_d{thd}"] = rd(SHAPES[n])
    assert raw.read() == b""
    return o


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", required=True, help="the reference's GEOSsatsim_GridComp directory")
    ap.add_argument("--work", default=None)
    ap.add_argument("--out", default=U.FIXTURE)
    ap.add_argument("--fc", default="/opt/rocm/lib/llvm/bin/flang")
    a = ap.parse_args()
    work = a.work or tempfile.mkdtemp(prefix="satsim_fixture_")
    b = U.make_batch(NP, NL)
    r4, r8 = (run(build(a.ref, work, k, a.fc), k, b) for k in ("r4", "r8"))
    fix = {f"in_{k}": v for k, v in b.items()}
    fix["in_emsfc_lw"] = np.float32(U.EMSFC_LW); fix["ncol"] = np.int32(NC)
    for ov in (1, 2, 3):
        assert np.array_equal(r4[f"mask_ov{ov}"], r8[f"mask_ov{ov}"]) and np.array_equal(r4[f"seed_ov{ov}"], r8[f"seed_ov{ov}"]), ov
    types = set()
    for th, thd in U.OPTION_PAIRS:
        s = f"_th{th}_d{thd}"
        b4, b8 = U.bins_of(r4["boxtau" + s], r4["boxptop" + s]), U.bins_of(r8["boxtau" + s], r8["boxptop" + s])
        moved = int(((b4[0] != b8[0]) | (b4[1] != b8[1])).sum())
        print(s, "cloudy sub-columns", int((b4[0] > 0).sum()), "moved between r4 and r8:", moved)
        assert moved == 0, "change the batch, not the bound"
        types |= set(zip(b4[0][b4[0] > 0].tolist(), b4[1][b4[0] > 0].tolist()))
        for n in U.CONTINUOUS:
            a4, a8 = r4[n + s].astype(np.float64), r8[n + s]
            assert np.array_equal(r4[n + s] == np.float32(U.MISSING), a8 == U.MISSING), (n, s)
            ok = a8 != U.MISSING
            fix["spread_" + n + s] = np.float64(np.abs(a4 - a8)[ok].max() if ok.any() else 0.0)
    print("cloud types populated:", len(types))
    for kind, ref, dt in (("r4", r4, np.float32), ("r8", r8, np.float64)):
        for ov in (1, 2, 3):
            m, sd = U.scops(b["seed"], b["cc"], b["conv"], ov, NC, dt)
            assert np.array_equal(m, ref[f"mask_ov{ov}"]) and np.array_equal(sd, ref[f"seed_ov{ov}"]), (kind, ov)
        for th, thd in U.OPTION_PAIRS:
            s = f"_th{th}_d{thd}"
            o = U.icarus(b["sunlit"], b["pfull"], b["phalf"], b["qv"], b["cc"], b["conv"], b["dtau_s"], b["dtau_c"], th, thd, 3, r4["mask_ov3"], b["skt"],
                         U.EMSFC_LW, b["at"], b["dem_s"], b["dem_c"], dt)
            assert np.array_equal(o["fq_isccp"], ref["fq_isccp" + s]), (kind, s)
            for n in U.CONTINUOUS:
                assert np.array_equal(o[n] == dt(U.MISSING), ref[n + s] == dt(U.MISSING)), (kind, n, s)
                ok = ref[n + s] != dt(U.MISSING)
                dd = np.abs(o[n].astype(np.float64) - ref[n + s].astype(np.float64))[ok]; rr = np.abs(ref[n + s].astype(np.float64)[ok])
                assert (dd[rr == 0] == 0).all()
                if kind == "r8":
                    fix["restate64_" + n + s] = np.float64(dd.max() if dd.size else 0.0)
                    fix["restate64rel_" + n + s] = np.float64((dd[rr > 0] / rr[rr > 0]).max() if (rr > 0).any() else 0.0)
    for kind, ref in (("r4", r4), ("r8", r8)):
        for k, v in ref.items():
            if k.startswith("mask_ov"):
                if kind == "r4":
                    fix[k] = v
            else:
                fix[f"{kind}_{k}"] = v
    np.savez_compressed(a.out, **fix)
    print("wrote", a.out, os.path.getsize(a.out), "bytes,", len(fix), "arrays")


if __name__ == "__main__":
    main()
