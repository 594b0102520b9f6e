"""The quad kernels (csrc/quad.hip) in the code the compiler emits (CPU; hipcc cross-compiles without a GPU).

Their design rests on two things the source cannot show: a register budget (pair A's valid half waits in 16 registers
through pair B's transform, at the waves per SIMD of the pair kernel of the same size) and two hand-counted
`s_waitcnt vmcnt(N)` per block, which are only right while there is no spill, exactly N stores follow each asm prefetch on
every path to its wait, and nothing touches the prefetch registers in between (scripts/audit_ps_isa.py, audit_quad)."""
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

QUAD = r"k_(fwd|inv)_quad_psILi(\d+)E"


@pytest.fixture(scope="module")
def listing(tmp_path_factory):
    if not shutil.which("hipcc"):
        pytest.skip("no hipcc on this machine")
    return audit_ps_isa.compile_to_asm(str(tmp_path_factory.mktemp("isa") / "quad.s"), "quad.hip")


@pytest.fixture(scope="module")
def usage():
    if not shutil.which("hipcc"):
        pytest.skip("no hipcc on this machine")
    sys.path.insert(0, ROOT)
    b = importlib.import_module("foo_dsp_bfir_amd._build")
    b.build()
    u = b.resource_usage()
    if not any(re.search(QUAD, k) for k in u):               # objects from a build that did not record it
        b.build(force=True)
        u = b.resource_usage()
    return u


def test_quad_kernels_have_no_scratch(usage):
    quads = {k: v for k, v in usage.items() if re.search(QUAD, k)}
    assert sorted(re.search(QUAD, k).groups() for k in quads) == [("inv", "13"), ("inv", "14")], sorted(quads)
    for name, r in quads.items():
        assert r["ScratchSize"] == 0 and r["VGPRs Spill"] == 0 and r["Dynamic Stack"] == "False", (name, r)


def test_every_quad_kernel_keeps_the_occupancy_of_its_pair_kernel(usage):
    """Waves per SIMD in the compiler's report, against k_inv_pair_ps of the same size, for whatever is instantiated.

    N = 8192 and 16384: 4 against 4 (124 / 128 registers against 91 / 91).  A size that cannot hold this is not
    instantiated and stays on the pair kernel (quad.hip): N = 1024 would reach 4 waves (123 registers) against 5 (89) --
    compiled for five it spills 77 registers --, N = 2048 / 4096 spill at their pair kernels' 4 / 3."""
    sizes = sorted(int(re.search(QUAD, k).group(2)) for k in usage if re.search(QUAD, k))
    assert 13 in sizes
    for size in sizes:
        _check_occupancy(usage, size)


def _check_occupancy(usage, size):
    quad = [v for k, v in usage.items() if re.search(r"k_inv_quad_psILi%dE" % size, k)]
    pair = [v for k, v in usage.items() if re.search(r"k_inv_pair_psILi%dE" % size, k)]
    assert len(quad) == 1 and len(pair) == 1
    print("N = 2^%d: quad %d waves, %d registers; pair %d waves, %d registers"
          % (size, quad[0]["Occupancy"], quad[0]["VGPRs"], pair[0]["Occupancy"], pair[0]["VGPRs"]))
    assert quad[0]["Occupancy"] >= pair[0]["Occupancy"], (quad[0], pair[0])


def test_quad_kernels_pass_the_audit(listing):
    rep = audit_ps_isa.audit_quad(listing)
    assert "k_inv_quad_ps<13>" in rep, sorted(rep)
    assert all(not errs for errs in rep.values()), {k: v for k, v in rep.items() if v}


def test_quad_auditor_catches_violations(listing, tmp_path):
    text = open(listing).read()
    name = re.search(r"^(_ZN4bfir\S*k_inv_quad_psILi13E\S*):", text, re.M).group(1)
    a = text.index(name + ":")
    b = text.index(".Lfunc_end", a)
    body = text[a:b]
    stores = [m.start() for m in re.finditer(r"\tbuffer_store_dwordx4 ", body)]
    assert len(stores) == 8                                  # eight 16-byte pieces per thread and block
    loads = [m.start() for m in re.finditer(r";;#ASMSTART\n(?:\ts_nop 4\n)?\tbuffer_load_dwordx4 ", body)]
    assert len(loads) == 2                                   # pair B under A's passes, the next block's pair A under B's

    def run(mutated_body, meta_edit=None):
        t = text[:a] + mutated_body + text[b:]
        if meta_edit:
            t = meta_edit(t)
        p = tmp_path / "m.s"
        p.write_text(t)
        return audit_ps_isa.audit_quad(str(p))["k_inv_quad_ps<13>"]

    assert run(body) == []
    # a ninth vector-memory operation inside the window of eight (what a spill would be)
    extra = body[:stores[3]] + "\tscratch_store_dword off, v1, off\n" + body[stores[3]:]
    assert any("carries 9 vector-memory ops" in e for e in run(extra))
    # one store fewer
    line_end = body.index("\n", stores[0])
    assert any("carries 7" in e for e in run(body[:stores[0]] + body[line_end + 1:]))
    # a vector-memory operation inside the window of none: between the first prefetch and the vmcnt(0) behind it
    end0 = body.index(";;#ASMEND", loads[0]) + len(";;#ASMEND\n")
    assert any("carries 1 vector-memory ops" in e for e in run(body[:end0] + "\tscratch_load_dword v1, off, off\n" + body[end0:]))
    # a copy out of a prefetch destination register before its wait, for either statement
    for at in loads:
        dest = re.match(r";;#ASMSTART\n(?:\ts_nop 4\n)?\tbuffer_load_dwordx4 v\[(\d+):", body[at:]).group(1)
        end = body.index(";;#ASMEND", at) + len(";;#ASMEND\n")
        touched = body[:end] + "\tv_mov_b32_e32 v0, v%s\n" % dest + body[end:]
        assert any("touched before its wait" in e for e in run(touched))
    # a spill recorded in the kernel's metadata
    def spill(t):
        i = t.index(".name:           " + name)
        j = t.index(".vgpr_spill_count: 0", i)
        return t[:j] + ".vgpr_spill_count: 2" + t[j + len(".vgpr_spill_count: 0"):]
    assert any(".vgpr_spill_count = 2" in e for e in run(body, spill))


def test_pair_audit_is_unchanged_by_the_quad_entry_point(listing):
    """audit() and parse() see the pair and time-pair kernels only: none of them lives in quad.hip"""
    assert audit_ps_isa.audit(listing) == {}
    assert audit_ps_isa.parse(listing)[0] == {}
