"""The C++ host mirror on a multi-level mimo engine: tests/cpp/test_mimo_levels_mirror.cpp built against the library and run."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cpp_mirror_runs_a_multi_level_mimo_engine(tmp_path, bfir):
    """10 -> 12 at L = 64 on two levels through the brutefir class; the program compares its output byte for byte with an
    engine made through the C ABI, and checks the delay refusal."""
    src = os.path.join(ROOT, "tests", "cpp", "test_mimo_levels_mirror.cpp")
    exe = str(tmp_path / "test_mimo_levels_mirror")
    libdir = os.path.dirname(bfir.library_path())
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", src, "-o", exe, "-L" + libdir, "-lbfir_hip",
                    "-Wl,-rpath," + libdir], check=True)
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(p.stdout[-2000:], p.stderr[-2000:])
    assert p.returncode == 0 and "ALL OK" in p.stdout
