"""CPU test of the sliding ring round's seam launch rule (federated_amd/csrc/cfa_slide_shape.h,
slide_takes_seam): built here without HIP from tests/native/slide_seam_shape_test.cpp and run.
Only a full ring walked in one segment with a window to retain takes the seam kernel, at a tile
width that has one (after the short-row step-down); partial runs, several segments and an empty
window take the plain kernel. The retained rows' LDS share lets the workgroups the kernel is held
to sit on one CU."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "slide_seam_shape_test.cpp")
INC = os.path.join(ROOT, "federated_amd", "csrc")

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")


def test_slide_seam_launch_rule(tmp_path):
    exe = str(tmp_path / "slide_seam_shape_test")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", f"-I{INC}", SRC, "-o", exe],
                   check=True, capture_output=True, text=True)
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and "OK" in p.stdout, p.stdout[-4000:] + p.stderr[-2000:]
