"""The C++ host mirror's bank mixes on a multi-level engine: tests/cpp/test_lbankmix_mirror.cpp built against the library and
run."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cpp_mirror_runs_mixes_of_a_levels_bank(tmp_path, bfir):
    """6 -> 6 at L = 256 on two levels through the brutefir class: the four mix methods on one engine, the _levels_bank
    methods on a twin whose bank holds every mix as an entry; the program compares the two engines' output bytes after every
    change, and a mix of two different entries against the same sum loaded as taps."""
    src = os.path.join(ROOT, "tests", "cpp", "test_lbankmix_mirror.cpp")
    exe = str(tmp_path / "test_lbankmix_mirror")
    libdir = os.path.dirname(bfir.library_path())
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", src, "-o", exe, "-L" + libdir, "-lbfir_hip",
                    "-Wl,-rpath," + libdir], check=True)
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(p.stdout[-2000:], p.stderr[-2000:])
    assert p.returncode == 0 and "ALL OK" in p.stdout
