"""The C++ host mirror's coefficient bank on a multi-level engine: tests/cpp/test_lbank_mirror.cpp built against the library
and run."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cpp_mirror_runs_a_levels_bank(tmp_path, bfir):
    """10 -> 10 at L = 256 on two levels through the brutefir class: the bank's methods on one engine, the calls with taps on
    a twin; the program compares the two engines' output bytes after every change, a plain and a fading pairs change among
    them."""
    src = os.path.join(ROOT, "tests", "cpp", "test_lbank_mirror.cpp")
    exe = str(tmp_path / "test_lbank_mirror")
    libdir = os.path.dirname(bfir.library_path())
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", src, "-o", exe, "-L" + libdir, "-lbfir_hip",
                    "-Wl,-rpath," + libdir], check=True)
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(p.stdout[-2000:], p.stderr[-2000:])
    assert p.returncode == 0 and "ALL OK" in p.stdout
