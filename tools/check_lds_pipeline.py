"""Static check of the hand-pipelined LDS fragment reads in the compiled conv3x3_mfma kernels.

conv3x3_mfma.h issues its `ds_read_b128` fragment reads through inline asm several reads ahead of their use and retires
them with counted `s_waitcnt lgkmcnt(N)`.  Between the read and the wait the compiler believes the destination VGPRs
already hold the data; if register pressure makes it copy or spill such a register (v_accvgpr_write, scratch_store,
v_mov ...) before the wait, it moves stale data.  This script compiles a .hip file to gfx950 assembly and verifies, per
kernel, that no instruction touches the destination of an in-flight asm read before a wait has retired it, and that
no asm read is carried around a loop: forward skips are covered by the linear scan, and a backward branch taken with reads in
flight (a join block or the top of a rotated loop placed above the branch) is followed from its target, with the state at the
branch, until those reads have been retired.

Second rule (round 2): MATRIX-OPERAND PROVENANCE.  The wrong sums round 1 recorded for the pipelined one-wave-per-SIMD fp32
ACCIN kernel were traced (tools/gpu_accin_probe2.py + the ISA) to a register-allocation miscompile of hipcc (ROCm 7.2), not
to the pipeline: with all 512 registers in use and weights shuttling through scratch and AGPRs, the 128-bit weight fragment
w[tap 0][k-group 0] was split into {scratch slot (x, y), a141 (z), a140 (w)}; phase 0 of the three-way unrolled walk
reassembles it correctly, phases 1 and 2 reload (x, y), copy w -- and never copy z: their first MFMAs read an accumulator
register that still holds element z of ANOTHER fragment, written by phase 0.  The in-flight rule cannot see that (no LDS
destination is touched).  What makes it visible statically: the MFMAs that consume the 2 or 4 elements of one LDS fragment
(consecutive registers of one asm read, same accumulator) take the matching elements of ONE weight fragment as their other
operand.  Inside the main loop each of those weight registers is either loop-invariant (never written in the loop), or
written earlier in the same barrier-delimited phase (reloaded / copied), or carried over from another phase (a reload the
compiler hoisted).  A fragment group that MIXES "written in this phase" with "carried over from another phase" is a
half-reassembled fragment -- exactly the miscompile above -- and is reported.

usage: check_lds_pipeline.py file.hip [more.hip ...]      (exit code 1 on a violation)
"""
import os
import re
import subprocess
import sys
import tempfile

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REG = re.compile(r"\bv\[(\d+):(\d+)\]|\bv(\d+)\b")
LGKM = re.compile(r"lgkmcnt\((\d+)\)")
VMC = re.compile(r"vmcnt\((\d+)\)")
VMEM_OPS = ("buffer_load", "global_load", "scratch_load", "buffer_store", "global_store", "scratch_store", "buffer_atomic",
            "global_atomic", "flat_")


def regs_of(text):
    out = set()
    for m in REG.finditer(text):
        if m.group(3) is not None:
            out.add(int(m.group(3)))
        else:
            out.update(range(int(m.group(1)), int(m.group(2)) + 1))
    return out


def per_file_flags(path):
    """the FLAGS_<file stem> := ... line of the Makefile next to the source, so the checked code is the shipped code"""
    mk = os.path.join(os.path.dirname(os.path.abspath(path)), "Makefile")
    stem = os.path.splitext(os.path.basename(path))[0]
    if os.path.exists(mk):
        for line in open(mk):
            m = re.match(r"FLAGS_%s\s*:?=\s*(.*)" % re.escape(stem), line)
            if m:
                return m.group(1).split()
    return []


def compile_to_asm(path, remarks=False):
    """the gfx950 assembly of the file as the Makefile builds it; remarks: (assembly, the compiler's resource-usage remarks)"""
    with tempfile.NamedTemporaryFile(suffix=".s", delete=False) as f:
        out = f.name
    cmd = [HIPCC, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-S", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage",
           "-I" + os.path.join(ROOT, "include"), "-I" + os.path.dirname(os.path.abspath(path))] + per_file_flags(path) + ["-o", out, path]
    err = subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, text=True).stderr
    text = open(out).read()
    os.unlink(out)
    return (text, err) if remarks else text


def resource_usage(path):
    """(assembly, {kernel: {"VGPRs", "AGPRs", "ScratchSize [bytes/lane]"}}) of the file, from one compilation"""
    text, err = compile_to_asm(path, remarks=True)
    usage, name = {}, None
    for line in err.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            usage[name] = {}
            continue
        m = re.search(r"remark:\s+(VGPRs|AGPRs|ScratchSize \[bytes/lane\]): (\d+)", line)
        if m and name:
            usage[name][m.group(1)] = int(m.group(2))
    return text, usage


class _Lds:
    """issue-ordered outstanding operations of a wave: `queue` LDS ops (is_asm_read, dest regs, line no), `vqueue` vector-memory
    ops (vmcnt retires them in order): (is_asm_load, dest regs, line no)"""
    def __init__(self, queue=(), vqueue=(), in_asm=False):
        self.queue, self.vqueue, self.in_asm = list(queue), list(vqueue), in_asm

    def copy(self):
        return _Lds(self.queue, self.vqueue, self.in_asm)

    def inflight(self):
        return set().union(*[q[1] for q in self.queue if q[0]]) if self.queue else set()

    def vinflight(self):
        return set().union(*[q[1] for q in self.vqueue if q[0]]) if self.vqueue else set()


def _clean(raw):
    return raw.split(";")[0].strip() if not raw.strip().startswith(";;#") else raw.strip()


def _step(st, kernel, ln, line, violations):
    """one instruction (not a label, branch, kernel header or s_endpgm) against the state; returns the asm reads it issued"""
    if line.startswith(";;#ASMSTART"):
        st.in_asm = True
        return 0
    if line.startswith(";;#ASMEND"):
        st.in_asm = False
        return 0
    inflight, vinflight = st.inflight(), st.vinflight()
    m = LGKM.search(line)
    if line.startswith("s_waitcnt"):
        mv = VMC.search(line)
        if mv:
            n = int(mv.group(1))
            st.vqueue = st.vqueue[len(st.vqueue) - n:] if n else []
        if m:
            n = int(m.group(1))
            st.queue = st.queue[len(st.queue) - n:] if n < len(st.queue) else st.queue
            if n == 0:
                st.queue = []
        return 0
    if line.startswith("s_barrier"):
        return 0
    touched = regs_of(line)
    if st.in_asm and line.startswith("buffer_load"):     # asm global -> register load (wgrad_mfma.hip): same contract, on vmcnt
        dest = regs_of(line.split(",")[0])
        if dest & (vinflight | inflight):
            violations.append((kernel, ln, "asm buffer load overwrites an in-flight destination: " + line))
        if (regs_of(",".join(line.split(",")[1:])) & (vinflight | inflight)):
            violations.append((kernel, ln, "asm buffer load reads an in-flight destination: " + line))
        st.vqueue.append((True, dest, ln))
        return 1
    if touched & vinflight:
        violations.append((kernel, ln, "touches an in-flight buffer-load destination: " + line))
    if line.startswith(VMEM_OPS):
        st.vqueue.append((False, set(), ln))
    if st.in_asm and line.startswith("ds_read"):
        dest = regs_of(line.split(",")[0])
        if dest & inflight:
            violations.append((kernel, ln, "asm read overwrites an in-flight destination: " + line))
        st.queue.append((True, dest, ln))
        return 1
    if touched & inflight:
        violations.append((kernel, ln, "touches an in-flight LDS destination: " + line))
    if line.startswith("ds_"):
        st.queue.append((False, set(), ln))
    return 0


FOLLOW_LINES = 4000   # a followed path retires its reads within one step of a main loop; far below this


def _skips_to_join(lines, i, target):
    """lines[i - 1] is `s_cbranch_execz target`: True if it is the skip of an exec-masked block whose other end is an unconditional
    `s_branch target` -- an `if` whose join block was placed above it.  The masked block holds LDS stores the counted waits include
    and the kernels keep its mask non-empty, so the path is the one through the block (as for a forward skip, where the linear
    scan assumes the same) and the s_branch carries the state to the join."""
    for raw in lines[i:i + 60]:
        line = _clean(raw)
        if line.endswith(":") and not line.startswith(";;#"):
            return False
        if line.startswith("s_branch"):
            return line.split()[-1] == target
        if line.startswith("s_cbranch") or line.startswith("s_endpgm"):
            return False
    return False


def _follow(lines, label_at, kernel, start, st, seen, violations, origin):
    """The taken path of a BACKWARD branch that has asm LDS reads in flight (block placement puts a join block, or the top of a
    rotated loop, above the branch): walk it from the target with the state at the branch until every such read has been
    retired.  Forward conditional branches are passed as in the linear scan, forward unconditional ones are taken; a second
    backward branch is followed in turn, and a label met twice with reads still in flight is a loop that carries them."""
    i, budget = start, FOLLOW_LINES
    while i < len(lines) and budget > 0:
        raw = lines[i]
        line = _clean(raw)
        i += 1
        budget -= 1
        if not line or (line.endswith(":") and not line.startswith(";;#")):
            continue
        if raw.startswith("_Z") or line.startswith("s_endpgm"):
            return
        if line.startswith("s_cbranch") or line.startswith("s_branch"):
            target = line.split()[-1]
            t = label_at.get(target)
            if t is not None and t < i:                # backward again
                if line.startswith("s_cbranch_execz") and _skips_to_join(lines, i, target):
                    continue
                if target in seen:
                    violations.append((kernel, origin, "asm LDS read in flight around a loop (followed from here to line %d): %s" % (i, line)))
                    return
                _follow(lines, label_at, kernel, t, st.copy(), seen | {target}, violations, origin)
                if line.startswith("s_branch"):
                    return
            elif line.startswith("s_branch") and t is not None:
                i = t
            continue
        _step(st, kernel, i, line, violations)
        if not st.inflight():
            return
    violations.append((kernel, origin, "asm LDS read in flight across a backward branch and not retired within %d lines of its target" % FOLLOW_LINES))


def check_asm(text):
    """returns (kernels checked, asm reads seen, list of violations)"""
    violations, kernels, nreads = [], 0, 0
    lines = text.split("\n")
    label_at = {}
    for i, raw in enumerate(lines):
        line = _clean(raw)
        if line.endswith(":") and not line.startswith(";;#"):
            label_at[line[:-1]] = i
    kernel, st, labels = None, _Lds(), set()
    for ln, raw in enumerate(lines, 1):
        line = _clean(raw)
        if raw.startswith("_Z") and raw.rstrip().split(";")[0].rstrip().endswith(":"):
            kernel, st, labels = raw.split(":")[0], _Lds(), set()
            kernels += 1
            continue
        if kernel is None or not line:
            continue
        if line.startswith("s_endpgm"):            # one exit of possibly several: what follows is reached by branches only
            st = _Lds()
            continue
        if line.startswith(".Lfunc_end"):
            kernel = None
            continue
        if line.endswith(":") and not line.startswith(";;#"):   # label: a forward skip lands here, the linear scan covers both paths
            labels.add(line[:-1])
            continue
        if line.startswith("s_cbranch") or line.startswith("s_branch"):
            target = line.split()[-1]
            if st.inflight() and target in labels and line.startswith("s_cbranch_execz") and _skips_to_join(lines, ln, target):
                continue
            if st.inflight() and target in labels:     # backward branch: a loop, or a block placed above its predecessor
                _follow(lines, label_at, kernel, label_at[target], st.copy(), {target}, violations, ln)
                if line.startswith("s_branch"):        # nothing falls through: the state went with the branch
                    st.queue = [(False, set(), q[2]) for q in st.queue]
            if st.vinflight() and target in labels:
                violations.append((kernel, ln, "asm buffer load in flight across a loop back-edge: " + line))
            continue
        nreads += _step(st, kernel, ln, line, violations)
    return kernels, nreads, violations


AREG = re.compile(r"\b([av])\[(\d+):(\d+)\]|\b([av])(\d+)\b")


def _regs(tok):
    out = set()
    for m in AREG.finditer(tok):
        if m.group(4) is not None:
            out.add((m.group(4), int(m.group(5))))
        else:
            out.update((m.group(1), r) for r in range(int(m.group(2)), int(m.group(3)) + 1))
    return out


def check_operand_provenance(text):
    """returns (kernels with a main loop, MFMAs checked, violations): see the module docstring, second rule."""
    violations, nk, nm = [], 0, 0
    lines = text.split("\n")
    starts = [i for i, l in enumerate(lines) if l.startswith("_Z") and l.rstrip().split(";")[0].rstrip().endswith(":")]
    for st in starts:
        try:
            en = next(i for i in range(st, len(lines)) if lines[i].strip().startswith("s_endpgm"))
        except StopIteration:
            continue
        body = [l.split(";")[0].strip() if not l.strip().startswith(";;#") else "" for l in lines[st:en]]
        label_at = {l[:-1]: i for i, l in enumerate(body) if l.endswith(":") and not l.startswith("_Z")}
        # outermost loop that contains MFMAs: widest backward branch span
        loop = None
        for i, l in enumerate(body):
            if l.startswith(("s_cbranch", "s_branch")):
                tgt = l.split()[-1]
                j = label_at.get(tgt)
                if j is not None and j < i and any(b.startswith("v_mfma") for b in body[j:i]):
                    if loop is None or (i - j) > (loop[1] - loop[0]):
                        loop = (j, i)
        if loop is None:
            continue
        nk += 1
        lo, hi = loop
        bars = [i for i in range(lo, hi + 1) if body[i].startswith("s_barrier")]
        bounds = [lo] + bars + [hi + 1]
        seg_of = {}
        for k in range(len(bounds) - 1):
            for i in range(bounds[k], bounds[k + 1]):
                seg_of[i] = k
        written = {}                       # reg -> set of segments where it is written inside the loop
        writes_before = {}                 # (segment, reg) -> first line of a write
        for i in range(lo, hi + 1):
            l = body[i]
            if not l or l.endswith(":") or l.startswith(("s_", ";", ".")):
                continue
            toks = l.split(None, 1)
            if len(toks) < 2:
                continue
            if toks[0].startswith(("global_store", "scratch_store", "ds_write", "buffer_store", "global_atomic")):
                continue
            for r in _regs(toks[1].split(",")[0]):
                written.setdefault(r, set()).add(seg_of[i])
                writes_before.setdefault((seg_of[i], r), i)
        # asm-read destination tuples (fragments) by register
        frag_of = {}
        for i in range(lo, hi + 1):
            if body[i].startswith("ds_read_b128") or body[i].startswith("ds_read_b64"):
                dst = sorted(_regs(body[i].split(None, 1)[1].split(",")[0]))
                for r in dst:
                    frag_of[r] = dst[0]
        groups = {}                        # (segment, accumulator, fragment base, ordinal of that fragment's reuse) -> statuses
        seen = {}
        for i in range(lo, hi + 1):
            l = body[i]
            if l.startswith("ds_read"):
                for r in _regs(l.split(None, 1)[1].split(",")[0]):
                    seen[frag_of.get(r, r)] = seen.get(frag_of.get(r, r), 0) + 1
                continue
            if not l.startswith("v_mfma"):
                continue
            ops = [t.strip() for t in l.split(None, 1)[1].split(",")]
            nm += 1
            ra, rb = sorted(_regs(ops[1])), sorted(_regs(ops[2]))
            # which operand is the LDS fragment?  (weights are the A operand in conv3x3_mfma / conv_split, B in wgrad)
            fa, fb = [r for r in ra if r in frag_of], [r for r in rb if r in frag_of]
            frag, other = (fb, ra) if fb else (fa, rb)
            if not frag:
                continue
            key = (seg_of[i], ops[0], frag_of[frag[0]], seen.get(frag_of[frag[0]], 0))
            for r in other:
                segs = written.get(r)
                if not segs:
                    st_ = "invariant"
                else:
                    w = writes_before.get((seg_of[i], r))
                    st_ = "phase" if (w is not None and w < i) else "carried"
                groups.setdefault(key, []).append((st_, r, i, l))
        for key, items in groups.items():
            kinds = {k for k, _, _, _ in items}
            if "phase" in kinds and "carried" in kinds:
                for k, r, i, l in items:
                    if k == "carried":
                        violations.append((lines[st].split(":")[0], st + i + 1,
                                           f"weight register {r[0]}{r[1]} is carried over from another loop phase while the rest of its "
                                           f"fragment was rewritten in this phase: {l}"))
    return nk, nm, violations


def main(paths):
    bad = 0
    for p in paths:
        asm = compile_to_asm(p)
        kernels, nreads, violations = check_asm(asm)
        nk, nm, v2 = check_operand_provenance(asm)
        violations = violations + v2
        print(f"{os.path.basename(p)}: {kernels} kernels, {nreads} pipelined LDS reads, {nm} loop MFMAs in {nk} kernels, "
              f"{len(violations)} violations")
        for k, ln, msg in violations[:20]:
            print(f"  {k[:90]} line {ln}: {msg}")
        bad += len(violations)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
