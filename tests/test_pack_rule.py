"""The one cells-per-lane rule of the record units (csrc/mlx_record.hpp: pack_width), checked by a
stand-alone host program against its statement: tests/native/pack_rule.cpp.  No GPU, no library."""

import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_pack_width_is_rule_a(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = str(tmp_path / "pack_rule")
    src = os.path.join(ROOT, "tests", "native", "pack_rule.cpp")
    build = subprocess.run([hipcc, "-x", "hip", "--cuda-host-only", "-O1", "-std=c++17", src, "-o", exe],
                           capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-2000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0 and "pack_rule OK" in run.stdout, run.stdout[-2000:] + run.stderr[-2000:]
