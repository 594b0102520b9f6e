"""The wide forward kernel (csrc/wide.hip) in the code the compiler emits (CPU; hipcc cross-compiles without a GPU).

Its design rests on two things the source cannot show: a register budget (both pairs' carried half-window, pair B's raw half
under pair A's passes and the prefetch of the next block under pair B's, at the waves per SIMD of the pair kernel of the same
size) and one hand-counted `s_waitcnt vmcnt(8)` per block, which is only right while there is no spill, exactly pair B's eight
spectrum stores follow the asm prefetch on every path to the wait, and nothing touches the prefetch registers in between
(scripts/audit_ps_isa.py, audit_wide)."""
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

WIDE = r"k_(fwd|inv)_wide_psILi(\d+)E"


def _listing(tmp_path_factory, source):
    if not shutil.which("hipcc"):
        pytest.skip("no hipcc on this machine")
    return audit_ps_isa.compile_to_asm(str(tmp_path_factory.mktemp("isa") / source.replace(".hip", ".s")), source)


@pytest.fixture(scope="module")
def listing(tmp_path_factory):
    return _listing(tmp_path_factory, "wide.hip")


@pytest.fixture(scope="module")
def usage():
    if not shutil.which("hipcc"):
        pytest.skip("no hipcc on this machine")
    sys.path.insert(0, ROOT)
    b = importlib.import_module("foo_dsp_bfir_amd._build")
    b.build()
    u = b.resource_usage()
    if not any(re.search(WIDE, k) for k in u):               # objects from a build that did not record it
        b.build(force=True)
        u = b.resource_usage()
    return u


def _sizes(usage):
    assert all(re.search(WIDE, k).group(1) == "fwd" for k in usage if re.search(WIDE, k))
    return sorted(int(re.search(WIDE, k).group(2)) for k in usage if re.search(WIDE, k))


def test_wide_kernels_have_no_scratch(usage):
    wides = {k: v for k, v in usage.items() if re.search(WIDE, k)}
    sizes = _sizes(usage)
    assert 13 in sizes and 14 in sizes and 12 not in sizes, sizes
    for name, r in wides.items():
        assert r["ScratchSize"] == 0 and r["VGPRs Spill"] == 0 and r["Dynamic Stack"] == "False", (name, r)


def test_every_wide_kernel_keeps_the_occupancy_of_its_pair_kernel(usage):
    """Waves per SIMD in the compiler's report, against k_fwd_pair_ps of the same size, for whatever is instantiated.

    N = 8192 and 16384: 4 against 4 (118 registers against 87 / 88).  A size that cannot hold this is not instantiated
    and stays on the pair kernel (wide.hip): N = 1024 and 2048 have no scratch at four waves (118 / 126 registers), but
    their pair kernels reach five (87 / 94); N = 4096 spills at four."""
    for size in _sizes(usage):
        wide = [v for k, v in usage.items() if re.search(r"k_fwd_wide_psILi%dE" % size, k)]
        pair = [v for k, v in usage.items() if re.search(r"k_fwd_pair_psILi%dE" % size, k)]
        assert len(wide) == 1 and len(pair) == 1
        print("N = 2^%d: wide %d waves, %d registers, %d bytes of LDS; pair %d waves, %d registers, %d bytes of LDS"
              % (size, wide[0]["Occupancy"], wide[0]["VGPRs"], wide[0]["LDS Size"],
                 pair[0]["Occupancy"], pair[0]["VGPRs"], pair[0]["LDS Size"]))
        assert wide[0]["Occupancy"] >= pair[0]["Occupancy"], (wide[0], pair[0])


def test_wide_kernels_pass_the_audit(listing):
    rep = audit_ps_isa.audit_wide(listing)
    assert "k_fwd_wide_ps<13>" in rep and "k_fwd_wide_ps<14>" in rep, sorted(rep)
    assert all(not errs for errs in rep.values()), {k: v for k, v in rep.items() if v}


def _bodies(text):
    """{mangled name: (start, end)} of the wide kernels' bodies in a listing"""
    out = {}
    for m in re.finditer(r"^(_ZN4bfir\S*k_fwd_wide_psILi\d+E\S*):", text, re.M):
        out[m.group(1)] = (m.start(), text.index(".Lfunc_end", m.start()))
    return out


def test_sixteen_byte_stores_are_not_followed_by_a_write_of_their_data(listing):
    """No VALU write of a data register of any 16-byte store in the slot behind it (cdna_hip_programming.md 5.7 item 1,
    stores; the store k_inv_quad_ps once got wrong, quad.hip).  The asm statement of the history stores ends in a wait state
    of its own; this holds the spectrum stores, which the compiler schedules, to the same."""
    text = open(listing).read()
    bodies = _bodies(text)
    assert len(bodies) >= 2
    for name, (a, b) in bodies.items():
        ins = [ln.split(";")[0].strip() for ln in text[a:b].splitlines()]
        ins = [t for t in ins if t and not t.startswith(".") and not t.endswith(":")]
        n_x4 = 0
        for i, t in enumerate(ins[:-1]):
            if not t.startswith("buffer_store_dwordx4"):
                continue
            n_x4 += 1
            data = audit_ps_isa.vregs(t.split(",")[0])
            nxt = ins[i + 1]
            if nxt.startswith("v_") and not nxt.startswith("v_cmp"):
                assert not (audit_ps_isa.vregs(nxt.split(",")[0]) & data), (name, t, nxt)
        assert n_x4 == 16 + 8 + 8        # the spectrum stores of both pairs, the history stores in the loop and ahead of it


def test_wide_auditor_catches_violations(listing, tmp_path):
    text = open(listing).read()
    name = re.search(r"^(_ZN4bfir\S*k_fwd_wide_psILi13E\S*):", text, re.M).group(1)
    a = text.index(name + ":")
    b = text.index(".Lfunc_end", a)
    body = text[a:b]
    loads = [m.start() for m in re.finditer(r";;#ASMSTART\n(?:\ts_nop 4\n)?\tbuffer_load_dwordx4 ", body)]
    assert len(loads) == 1                                   # ONE prefetch statement per block, both pairs ...
    end = body.index(";;#ASMEND", loads[0]) + len(";;#ASMEND\n")
    assert len(re.findall(r"\tbuffer_load_dwordx4 ", body[loads[0]:end])) == 8          # ... of eight 16-byte loads
    assert len(re.findall(r"\tbuffer_load_dwordx4 [^\n]*\n", body[end:])) == 0
    # pair B's eight spectrum stores: the nontemporal 16-byte stores behind the prefetch (pair A's lie ahead of it; the
    # history stores, an asm statement behind the wait, are not nontemporal)
    stores = [m.start() for m in re.finditer(r"\tbuffer_store_dwordx4 [^\n]* nt\n", body) if m.start() > end]
    assert len(stores) == 8 and len(re.findall(r"\tbuffer_store_dwordx4 [^\n]* nt\n", body[:end])) == 8

    def run(mutated_body, meta_edit=None):
        t = text[:a] + mutated_body + text[b:]
        if meta_edit:
            t = meta_edit(t)
        p = tmp_path / "m.s"
        p.write_text(t)
        return audit_ps_isa.audit_wide(str(p))["k_fwd_wide_ps<13>"]

    assert run(body) == []
    # a ninth vector-memory operation inside the window of eight (what a spill would be)
    extra = body[:stores[3]] + "\tscratch_store_dword off, v1, off\n" + body[stores[3]:]
    assert any("carries 9 vector-memory ops" in e for e in run(extra))
    # ... and one that is a load
    extra = body[:stores[3]] + "\tscratch_load_dword v1, off, off\n" + body[stores[3]:]
    assert any("carries 9 vector-memory ops, 8 of them stores" in e for e in run(extra))
    # one store fewer
    line_end = body.index("\n", stores[0])
    assert any("carries 7" in e for e in run(body[:stores[0]] + body[line_end + 1:]))
    # a copy out of a prefetch destination register before its wait
    dest = re.match(r";;#ASMSTART\n(?:\ts_nop 4\n)?\tbuffer_load_dwordx4 v\[(\d+):", body[loads[0]:]).group(1)
    touched = body[:end] + "\tv_mov_b32_e32 v0, v%s\n" % dest + body[end:]
    assert any("touched before its wait" in e for e in run(touched))
    # a spill recorded in the kernel's metadata
    def spill(t):
        i = t.index(".name:           " + name)
        j = t.index(".vgpr_spill_count: 0", i)
        return t[:j] + ".vgpr_spill_count: 2" + t[j + len(".vgpr_spill_count: 0"):]
    assert any(".vgpr_spill_count = 2" in e for e in run(body, spill))


def test_the_other_audits_do_not_see_the_wide_kernel(listing):
    """audit() and audit_quad() parse their own families only: nothing of wide.hip"""
    assert audit_ps_isa.audit(listing) == {}
    assert audit_ps_isa.parse(listing)[0] == {}
    assert audit_ps_isa.audit_quad(listing) == {}


def test_pair_and_quad_audits_are_unchanged(tmp_path_factory):
    """audit() on pair.hip and audit_quad() on quad.hip report what they reported before wide.hip: every pair and time-pair
    kernel of the five sizes and the two quad instantiations, no finding, and no wide kernel among them."""
    pair = audit_ps_isa.audit(_listing(tmp_path_factory, "pair.hip"))
    assert sorted(pair) == sorted("k_%s_%s_ps<%d>" % (d, f, n) for d in ("fwd", "inv") for f in ("pair", "tp") for n in range(10, 15))
    assert all(not errs for errs in pair.values()), {k: v for k, v in pair.items() if v}
    quad = audit_ps_isa.audit_quad(_listing(tmp_path_factory, "quad.hip"))
    assert sorted(quad) == ["k_inv_quad_ps<13>", "k_inv_quad_ps<14>"]
    assert all(not errs for errs in quad.values()), {k: v for k, v in quad.items() if v}
