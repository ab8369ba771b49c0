"""CPU test of the sliding ring round's tile-width rule (federated_amd/csrc/cfa_slide_shape.h,
slide_pick_u): built here without HIP from tests/native/slide_shape_test.cpp and run. The rule
never picks a tile width that leaves workgroups without a tile while a narrower one would fill
the device, keeps the tuned default at the bench's shape (25M fp32 rows, 256 CUs) and gives one
float4 per lane below one tile."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "slide_shape_test.cpp")
INC = os.path.join(ROOT, "federated_amd", "csrc")

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")


def test_slide_tile_width_rule(tmp_path):
    exe = str(tmp_path / "slide_shape_test")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", f"-I{INC}", SRC, "-o", exe],
                   check=True, capture_output=True, text=True)
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and "OK" in p.stdout, p.stdout[-4000:] + p.stderr[-2000:]
