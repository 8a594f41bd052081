"""CPU: the call records and tile tables of csrc/gridcomp_kernels.hpp are host code: tests/gridcomp_rules_check.hip carries the test of a tile's
description and the tile packing the SW drivers made before the tables existed and requires, case by case, the same (code, message) from lit_check
and the same LitScatter / SwdPostLit contents from swd_merge, lit_scatter_pack and post_lit_pack.  It ends with status 1 on the first difference,
on a message that no case produced, and on a sweep without an accepted case; the counts below are those of its sweeps."""
import os
import subprocess
from tests.conftest import ROOT

CASES = {"lit_check_swd": 20726, "lit_check_swc": 20330, "pack_swd": 6000, "pack_swc": 3000}


def test_the_tables_reject_and_pack_as_the_statements_they_replace(tmp_path):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    exe = str(tmp_path / "gridcomp_rules_check")
    subprocess.check_call([hipcc, "--offload-host-only", "-std=c++17", "-O1", os.path.join(ROOT, "tests", "gridcomp_rules_check.hip"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    got = {k: int(v) for k, v in (line.split() for line in out.stdout.splitlines())}
    assert got == dict(CASES, total=sum(CASES.values())), out.stdout
