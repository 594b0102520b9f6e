"""The C++ host mirror on a long-partition engine: tests/cpp/test_big_mirror.cpp built against the library and run."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cpp_mirror_runs_a_big_engine(tmp_path, bfir):
    """One big engine at L = 32768 through the brutefir class, one run() per block; the program checks a few output samples
    against the direct sum in double precision at the project's 1e-5."""
    src = os.path.join(ROOT, "tests", "cpp", "test_big_mirror.cpp")
    exe = str(tmp_path / "test_big_mirror")
    libdir = os.path.dirname(bfir.library_path())
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", src, "-o", exe, "-L" + libdir, "-lbfir_hip",
                    "-Wl,-rpath," + libdir], check=True)
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(p.stdout[-2000:], p.stderr[-2000:])
    assert p.returncode == 0 and "ALL OK" in p.stdout
