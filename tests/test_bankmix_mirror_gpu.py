"""The C++ host mirror's bank mixes: tests/cpp/test_bankmix_mirror.cpp built against the library and run."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cpp_mirror_mixes_a_bank(tmp_path, bfir):
    """10 -> 10 at L = 256 through the brutefir class: the four mix methods on one engine, the C calls on a second; the program
    compares the two engines' filter stores and output bytes after every change, and one row with the definition."""
    src = os.path.join(ROOT, "tests", "cpp", "test_bankmix_mirror.cpp")
    exe = str(tmp_path / "test_bankmix_mirror")
    libdir = os.path.dirname(bfir.library_path())
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", src, "-o", exe, "-L" + libdir, "-lbfir_hip",
                    "-Wl,-rpath," + libdir], check=True)
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(p.stdout[-2000:], p.stderr[-2000:])
    assert p.returncode == 0 and "ALL OK" in p.stdout
