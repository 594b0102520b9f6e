"""k_mac_stream<32, 8, false> (csrc/kernels.hip), the headline's MAC, in the code the compiler emits (CPU; hipcc
cross-compiles without a GPU), with the product's flags (_build.FLAGS).

Its time is vector issue: 128 FMAs per block-step, and whatever else a step holds is issued on top of them with two or three
waves per SIMD to hide behind.  The addressing through buffer descriptors (MacIo) leaves a step with a load, a store,
one wait and three scalar instructions (the delay line's offset with its wrap, the output's offset).

The parent of that change, same flags: 2357 instructions with a scalar mnemonic (`s_...`: 120 of them branches, 98 waits;
about 25 per block-step), 69 exec-mask saves, 357 vector instructions that are not FMAs, 6 scratch instructions and
ScratchSize 20 at 168 registers, occupancy 3 -- and 8210 FMAs: the 8192 of the three unrolled groups (528 + 1024 + 496
complex multiply-adds of four) and 18 in the DC | Nyquist chains of the first workgroups (two real chains, unrolled by
eight plus one; without -fno-slp-vectorize the compiler packs those two chains, and the count of the whole kernel is
8192)."""
import importlib
import importlib.util
import os
import re
import shutil
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
spec = importlib.util.spec_from_file_location("audit_ps_isa", os.path.join(ROOT, "scripts", "audit_ps_isa.py"))
audit_ps_isa = importlib.util.module_from_spec(spec)
spec.loader.exec_module(audit_ps_isa)

HEADLINE = r"k_mac_streamILi32ELi8ELb0E"
PARENT_SCALAR = 2357          # scalar mnemonics in the parent's kernel, branches among them
PARENT_BRANCHES = 120
GROUP_FMAS = 8192             # 32 x 32 complex multiply-adds over the three groups, four FMAs each
DC_NYQUIST_FMAS = 18          # the two real chains of bin 0 (not the streaming lanes' work)


@pytest.fixture(scope="module")
def body(tmp_path_factory):
    if not shutil.which("hipcc"):
        pytest.skip("no hipcc on this machine")
    text = open(audit_ps_isa.compile_to_asm(str(tmp_path_factory.mktemp("isa") / "kernels.s"), "kernels.hip")).read()
    names = re.findall(r"^(_ZN4bfir\S*%s\S*):" % HEADLINE, text, re.M)
    assert len(names) == 1, names
    a = text.index(names[0] + ":")
    return [ln.split()[0] for ln in text[a:text.index(".Lfunc_end", a)].splitlines()
            if ln.startswith("\t") and not ln.startswith(("\t.", "\t;"))]


def test_register_report_of_the_headline_mac():
    if not shutil.which("hipcc"):
        pytest.skip("no hipcc on this machine")
    sys.path.insert(0, ROOT)
    b = importlib.import_module("foo_dsp_bfir_amd._build")
    b.build()
    u = b.resource_usage()
    if not any(re.search(HEADLINE, k) for k in u):            # objects from a build that did not record it
        b.build(force=True)
        u = b.resource_usage()
    ks = {k: v for k, v in u.items() if re.search(HEADLINE, k)}
    assert len(ks) == 1, sorted(ks)
    for name, r in ks.items():
        print(name, r)
        assert r["ScratchSize"] == 0 and r["VGPRs Spill"] == 0 and r["Dynamic Stack"] == "False", (name, r)
        assert r["VGPRs"] <= 168 and r["Occupancy"] == 3, (name, r)


def test_scalar_instructions_and_branches_are_a_third_of_the_parents(body):
    scalar = sum(op.startswith("s_") for op in body)
    branches = sum(op.startswith(("s_cbranch", "s_branch")) for op in body)
    print("scalar mnemonics %d (parent %d), of them branches %d (parent %d)" % (scalar, PARENT_SCALAR, branches, PARENT_BRANCHES))
    # the branches are scalar mnemonics too: held once as part of the whole, and once counted twice as the issue adds them
    assert 3 * scalar <= PARENT_SCALAR
    assert 3 * (scalar + branches) <= PARENT_SCALAR + PARENT_BRANCHES


def test_the_fmas_are_the_parents(body):
    fmas = sum(op.startswith(("v_fma_f32", "v_fmac_f32")) for op in body)
    assert fmas - DC_NYQUIST_FMAS == GROUP_FMAS, fmas
