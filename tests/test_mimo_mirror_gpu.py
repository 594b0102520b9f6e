"""The C++ host mirror on a mimo engine: tests/cpp/test_mimo_mirror.cpp built against the library and run."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cpp_mirror_runs_a_mimo_engine(tmp_path, bfir):
    """12 -> 3 at L = 256 through the brutefir class; the program checks every output sample against the direct
    convolution in double precision at the project's 1e-5."""
    src = os.path.join(ROOT, "tests", "cpp", "test_mimo_mirror.cpp")
    exe = str(tmp_path / "test_mimo_mirror")
    libdir = os.path.dirname(bfir.library_path())
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", src, "-o", exe, "-L" + libdir, "-lbfir_hip",
                    "-Wl,-rpath," + libdir], check=True)
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(p.stdout[-2000:], p.stderr[-2000:])
    assert p.returncode == 0 and "ALL OK" in p.stdout
