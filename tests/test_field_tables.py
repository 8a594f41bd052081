"""CPU: the Fields<S> tables of csrc/gridcomp_kernels.hpp, which bind the public in[] / out[] pointer tables of the GridComp entry points
(include/geosrad.h, GEOSRAD_LWD_* ...) to the kernels' argument structs, are host code: tests/field_tables_check.hip binds a distinct pointer
per slot and names, member by member, the slot each one must have received.  A swapped entry, or one left empty, fails here."""
import os
import subprocess
from tests.conftest import ROOT


def test_every_table_entry_reaches_the_member_its_enum_names(tmp_path):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    exe = str(tmp_path / "field_tables_check")
    subprocess.check_call([hipcc, "--offload-host-only", "-std=c++17", "-O0", os.path.join(ROOT, "tests", "field_tables_check.hip"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    assert int(out.stdout.split()[0]) == 334, out.stdout
