"""csrc/coeff_tables.h without a GPU: the host arithmetic that turns the integers of a set call (pairs, bank entries, mix terms)
into the tables the kernels read.  tests/cpp/test_coeff_tables.cpp includes the header alone, is built with AddressSanitizer and
UndefinedBehaviorSanitizer and run as a plain executable; the header stays free of HIP, and engine.hip holds no second copy of
what it took over."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "foo-dsp-bfir_amd", "csrc")


def test_table_builders_under_the_host_sanitizers(tmp_path):
    if not shutil.which("g++"):
        pytest.skip("no g++ on this machine")
    src = os.path.join(ROOT, "tests", "cpp", "test_coeff_tables.cpp")
    exe = str(tmp_path / "test_coeff_tables")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g",
                    src, "-o", exe], check=True)
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(p.stdout[-4000:], p.stderr[-4000:])
    assert p.returncode == 0 and "ALL OK" in p.stdout and "FAIL" not in p.stdout
    assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr


def test_header_is_host_only_and_the_one_copy():
    header = open(os.path.join(CSRC, "coeff_tables.h")).read()
    engine = open(os.path.join(CSRC, "engine.hip")).read()
    includes = re.findall(r'^#\s*include\s+[<"]([^>"]+)[>"]', header, re.M)
    assert includes and not [i for i in includes if "hip/" in i or i in ("kernels.h",)], includes
    assert "bfir_engine" not in re.sub(r"//.*", "", header)                # plain ints and vectors, no engine
    assert '#include "coeff_tables.h"' in engine
    both = header + engine
    assert both.count("tab.push_back(i); tab.push_back") == 1            # one patch-table builder
    assert both.count("// the same pair twice") == 1                     # one list check
    assert not re.search(r"hipMalloc\(\(void \*\*\)&\w+->d_(gather|patch)\b", engine)   # the tables grow in upload_table alone
