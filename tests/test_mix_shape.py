"""CPU test of the streaming mixes' host-only launch rules (federated_amd/csrc/cfa_mix_shape.h):
built here without HIP from tests/native/mix_shape_test.cpp and run. The bucket split covers every
byte misalignment of three pointers at P = 0..40, the pass iterator every fan-in up to three full
passes and one neighbour, and the launch-shape bands are pinned at both sides of each edge."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "mix_shape_test.cpp")
INCS = [os.path.join(ROOT, "federated_amd", "csrc"), os.path.join(ROOT, "include")]

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")


def test_mix_shape_rules(tmp_path):
    exe = str(tmp_path / "mix_shape_test")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", *[f"-I{i}" for i in INCS], SRC, "-o", exe],
                   check=True, capture_output=True, text=True)
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and "OK" in p.stdout, p.stdout[-4000:] + p.stderr[-2000:]
