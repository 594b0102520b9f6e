#!/usr/bin/env python3
"""Machine check of the hand-counted vmcnt scheme of the persistent pair kernels (pair.hip).

k_fwd_pair_ps / k_inv_pair_ps (and their pairs-in-time siblings k_fwd_tp_ps / k_inv_tp_ps) issue the next block's buffer loads from an inline-asm statement the compiler's
s_waitcnt bookkeeping cannot see, and wait for them with a hand-written `s_waitcnt vmcnt(N)`, N = the vector-memory
stores issued after the prefetch.  That is only right while, in the code hipcc actually emits,

  1. the kernel has no scratch: vgpr/sgpr spill counts 0, private segment 0 (a spill is a VMEM op the count misses);
  2. on EVERY control-flow path from the prefetch statement to the counted in-loop wait there are exactly N
     vector-memory instructions, all of them stores, and N equals the wait's immediate;
  3. no instruction on any path from the prefetch to the wait that covers it (the counted one in the loop, the
     vmcnt(0) one behind it) reads or writes a prefetch destination register -- no copy, no reuse;
  4. there is exactly one prefetch statement, one counted wait and one closing vmcnt(0) wait per kernel.

hipcc cross-compiles without a GPU, so this runs in the CPU test suite (tests/test_isa_audit.py) and fails the build
when a compiler or flag change breaks an assumption.  BFIR_PAIR=0 (the planar staging kernels) is the fallback at run time.

k_inv_quad_ps (quad.hip) has two prefetch statements and two counted waits per block: audit_quad() checks 1 - 3 for each
window (tests/test_quad_isa.py); audit() and parse() see the pair and time-pair kernels only.

k_fwd_wide_ps (wide.hip) has ONE prefetch statement of eight loads (both channel pairs of the next block, issued under the
second pair's passes), one counted wait and one closing wait: audit_wide() holds it to 1 - 4 as they stand
(tests/test_wide_isa.py).

    python scripts/audit_ps_isa.py [pair.s]      (without an argument: compiles csrc/pair.hip, csrc/quad.hip and csrc/wide.hip
                                                  to assembly first)
"""
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VMEM = re.compile(r"^(buffer|global|flat|scratch)_(load|store|atomic)")
REG = re.compile(r"\bv(\d+)\b|\bv\[(\d+):(\d+)\]")


def compile_to_asm(out_path, source="pair.hip"):
    sys.path.insert(0, ROOT)
    from importlib import import_module
    b = import_module("foo_dsp_bfir_amd._build")
    src = os.path.join(b.CSRC, source)
    cmd = ["hipcc"] + b.FLAGS + ["-S", "--cuda-device-only", "-o", out_path, src]
    subprocess.run(cmd, check=True, stderr=subprocess.DEVNULL)
    return out_path


def vregs(text):
    s = set()
    for m in REG.finditer(text):
        if m.group(1) is not None:
            s.add(int(m.group(1)))
        else:
            s.update(range(int(m.group(2)), int(m.group(3)) + 1))
    return s


class Kernel:
    def __init__(self, name, lines):
        self.name = name
        self.ins = []          # (text, in_asm)
        self.labels = {}
        in_asm = False
        for ln in lines:
            t = ln.split(";")[0].strip() if not ln.strip().startswith(";;#") else ln.strip()
            if t.startswith(";;#ASMSTART"):
                in_asm = True
                continue
            if t.startswith(";;#ASMEND"):
                in_asm = False
                continue
            if not t or t.startswith("."):
                m = re.match(r"^(\.LBB\d+_\d+):", t)
                if m:
                    self.labels[m.group(1)] = len(self.ins)
                continue
            self.ins.append((t, in_asm))

    def succ(self, i):
        t = self.ins[i][0]
        if t.startswith("s_endpgm"):
            return []
        m = re.match(r"^s_branch\s+(\S+)", t)
        if m:
            return [self.labels[m.group(1)]]
        m = re.match(r"^s_cbranch_\w+\s+(\S+)", t)
        if m:
            return [self.labels[m.group(1)], i + 1]
        return [i + 1] if i + 1 < len(self.ins) else []


def audit_kernel(k, meta):
    errs = []
    for key in (".vgpr_spill_count", ".sgpr_spill_count", ".private_segment_fixed_size"):
        if meta.get(key, None) != 0:
            errs.append("%s = %r (must be 0)" % (key, meta.get(key)))
    pre = [i for i, (t, a) in enumerate(k.ins) if a and t.startswith("buffer_load")]
    waits = [(i, int(re.search(r"vmcnt\((\d+)\)", t).group(1))) for i, (t, a) in enumerate(k.ins)
             if a and t.startswith("s_waitcnt vmcnt")]
    if not pre:
        return ["no inline-asm prefetch found"]
    # one statement = consecutive asm loads
    if pre[-1] - pre[0] != len(pre) - 1 or len(pre) not in (8, 16):
        errs.append("expected ONE prefetch statement of 8 (or, pairs in time, 16) loads, found asm loads at %s" % pre)
    counted = [w for w in waits if w[1] > 0]
    closing = [w for w in waits if w[1] == 0]
    if len(counted) != 1 or len(closing) != 1:
        errs.append("expected one counted and one closing asm wait, found %s" % waits)
        return errs
    dests = set()
    for i in pre:
        dests |= vregs(k.ins[i][0].split(",")[0])
    wait_at = {w[0]: w[1] for w in waits}
    # every path from behind the prefetch to an asm wait
    start = pre[-1] + 1
    seen, stack, ends = set(), [(start, 0, 0)], {}
    while stack:
        i, n_vmem, n_store = stack.pop()
        if (i, n_vmem) in seen or n_vmem > 64:
            continue
        seen.add((i, n_vmem))
        t, in_asm = k.ins[i]
        if i in wait_at:
            ends.setdefault(i, set()).add((n_vmem, n_store))
            continue
        if in_asm and t.startswith("buffer_load"):
            errs.append("a path reaches the prefetch again without passing a wait (instruction %d)" % i)
            continue
        if not in_asm and not t.startswith("s_"):
            hit = vregs(t) & dests
            if hit:
                errs.append("prefetch destination v%s touched before its wait: `%s`" % (sorted(hit), t))
        if VMEM.match(t):
            n_vmem += 1
            n_store += 1 if "_store" in t else 0
        nxt = k.succ(i)
        if not nxt:
            errs.append("a path from the prefetch ends the program without a wait (`%s`)" % t)
        for j in nxt:
            stack.append((j, n_vmem, n_store))
    ci, cn = counted[0]
    if ci not in ends:
        errs.append("no path from the prefetch reaches the counted wait")
    else:
        for n_vmem, n_store in ends[ci]:
            if n_vmem != cn or n_store != n_vmem:
                errs.append("path to `s_waitcnt vmcnt(%d)` carries %d vector-memory ops, %d of them stores"
                            % (cn, n_vmem, n_store))
    if closing[0][0] not in ends:
        errs.append("no path from the prefetch reaches the closing vmcnt(0) wait")
    return errs


def parse(asm_path, family="pair|tp"):
    text = open(asm_path).read().splitlines()
    kernels, cur, name = {}, None, None
    for ln in text:
        m = re.match(r"^(_ZN4bfir\S*k_(?:fwd|inv)_(?:%s)_psILi\d+E\S*):" % family, ln)
        if m:
            name, cur = m.group(1), []
            continue
        if cur is not None:
            if ln.startswith("\t.section") or ln.startswith(".Lfunc_end"):
                kernels[name] = Kernel(name, cur)
                cur = None
            else:
                cur.append(ln)
    meta, kname = {}, None
    for ln in text:
        m = re.match(r"^\s+(?:- )?\.name:\s+(\S+)", ln)
        if m:
            kname = m.group(1)
            meta.setdefault(kname, {})
        m = re.match(r"^\s+(?:- )?(\.\w+):\s+(\d+)\s*$", ln)
        if m and kname:
            meta[kname][m.group(1)] = int(m.group(2))
    return kernels, meta


def audit(asm_path):
    kernels, meta = parse(asm_path)
    report = {}
    for name, k in sorted(kernels.items()):
        short = re.search(r"k_(fwd|inv)_(pair|tp)_psILi(\d+)E", name)
        report["k_%s_%s_ps<%s>" % short.groups()] = audit_kernel(k, meta.get(name, {}))
    return report


def audit_quad_kernel(k, meta):
    """The quad kernels (quad.hip) alternate two prefetch statements and two in-loop waits, one per channel pair, before the
    closing vmcnt(0).  Same properties as audit_kernel, per window: on every path from a prefetch statement to the first
    asm wait behind it the vector-memory operations are all stores and as many as that wait's count (the closing wait
    takes any number: it waits for all), and nothing on the way touches that statement's destination registers."""
    errs = []
    for key in (".vgpr_spill_count", ".sgpr_spill_count", ".private_segment_fixed_size"):
        if meta.get(key, None) != 0:
            errs.append("%s = %r (must be 0)" % (key, meta.get(key)))
    pre = [i for i, (t, a) in enumerate(k.ins) if a and t.startswith("buffer_load")]
    wait_at = {i: int(re.search(r"vmcnt\((\d+)\)", t).group(1)) for i, (t, a) in enumerate(k.ins)
               if a and t.startswith("s_waitcnt vmcnt")}
    stmts = []                                               # one statement = consecutive asm loads
    for i in pre:
        if stmts and i == stmts[-1][-1] + 1:
            stmts[-1].append(i)
        else:
            stmts.append([i])
    if len(stmts) != 2 or any(len(s) != 8 for s in stmts):
        return errs + ["expected TWO prefetch statements of 8 loads, found asm loads at %s" % pre]

    def reaches_prefetch(w):                                 # a wait inside the loop: the prefetch comes round again
        seen, stack = set(), list(k.succ(w))
        while stack:
            i = stack.pop()
            if i in seen:
                continue
            seen.add(i)
            if i in pre:
                return True
            stack.extend(k.succ(i))
        return False

    closing = [w for w in wait_at if not reaches_prefetch(w)]
    inloop = [w for w in wait_at if w not in closing]
    if len(inloop) != 2 or len(closing) != 1 or wait_at[closing[0]] != 0:
        return errs + ["expected two in-loop asm waits and one closing vmcnt(0), found %s" % sorted(wait_at.items())]
    reached = {}                                             # wait -> statements whose window ends there
    for n, stmt in enumerate(stmts):
        dests = set()
        for i in stmt:
            dests |= vregs(k.ins[i][0].split(",")[0])
        seen, stack, ends = set(), [(stmt[-1] + 1, 0, 0)], {}
        while stack:
            i, n_vmem, n_store = stack.pop()
            if (i, n_vmem) in seen or n_vmem > 64:
                continue
            seen.add((i, n_vmem))
            t, in_asm = k.ins[i]
            if i in wait_at:
                ends.setdefault(i, set()).add((n_vmem, n_store))
                continue
            if in_asm and t.startswith("buffer_load"):
                errs.append("a path from prefetch %d reaches a prefetch without passing a wait (instruction %d)" % (n, i))
                continue
            if not in_asm and not t.startswith("s_"):
                hit = vregs(t) & dests
                if hit:
                    errs.append("prefetch %d: destination v%s touched before its wait: `%s`" % (n, sorted(hit), t))
            if VMEM.match(t):
                n_vmem += 1
                n_store += 1 if "_store" in t else 0
            nxt = k.succ(i)
            if not nxt:
                errs.append("a path from prefetch %d ends the program without a wait (`%s`)" % (n, t))
            for j in nxt:
                stack.append((j, n_vmem, n_store))
        if not any(w in inloop for w in ends):
            errs.append("no path from prefetch %d reaches an in-loop wait" % n)
        for w, counts in ends.items():
            reached.setdefault(w, set()).add(n)
            for n_vmem, n_store in counts:
                if n_store != n_vmem or (w in inloop and n_vmem != wait_at[w]):
                    errs.append("path from prefetch %d to `s_waitcnt vmcnt(%d)` carries %d vector-memory ops, %d of them stores"
                                % (n, wait_at[w], n_vmem, n_store))
    for w in inloop:
        if len(reached.get(w, ())) != 1:
            errs.append("the in-loop wait vmcnt(%d) ends the windows of prefetches %s (must be exactly one)"
                        % (wait_at[w], sorted(reached.get(w, ()))))
    if closing[0] not in reached:
        errs.append("no path from a prefetch reaches the closing vmcnt(0) wait")
    return errs


def audit_quad(asm_path=None):
    """{"k_inv_quad_ps<13>": [errors], ...} for the quad kernels; without a listing, compiles csrc/quad.hip first."""
    if asm_path is None:
        asm_path = compile_to_asm(os.path.join(tempfile.mkdtemp(prefix="bfir_isa_"), "quad.s"), "quad.hip")
    kernels, meta = parse(asm_path, "quad")
    report = {}
    for name, k in sorted(kernels.items()):
        short = re.search(r"k_(fwd|inv)_quad_psILi(\d+)E", name)
        report["k_%s_quad_ps<%s>" % short.groups()] = audit_quad_kernel(k, meta.get(name, {}))
    return report


def audit_wide(asm_path=None):
    """{"k_fwd_wide_ps<13>": [errors], ...} for the wide kernels; without a listing, compiles csrc/wide.hip first."""
    if asm_path is None:
        asm_path = compile_to_asm(os.path.join(tempfile.mkdtemp(prefix="bfir_isa_"), "wide.s"), "wide.hip")
    kernels, meta = parse(asm_path, "wide")
    report = {}
    for name, k in sorted(kernels.items()):
        short = re.search(r"k_(fwd|inv)_wide_psILi(\d+)E", name)
        report["k_%s_wide_ps<%s>" % short.groups()] = audit_kernel(k, meta.get(name, {}))
    return report


def main():
    if len(sys.argv) > 1:
        path = sys.argv[1]
    else:
        path = compile_to_asm(os.path.join(tempfile.mkdtemp(prefix="bfir_isa_"), "pair.s"))
    rep = audit(path)
    rep.update(audit_quad(path if len(sys.argv) > 1 else None))
    rep.update(audit_wide(path if len(sys.argv) > 1 else None))
    bad = 0
    for k, errs in rep.items():
        print("%-24s %s" % (k, "ok" if not errs else "FAIL"))
        for e in errs:
            print("    " + e)
            bad += 1
    if not rep:
        print("no persistent pair kernels found in", path)
        return 1
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
