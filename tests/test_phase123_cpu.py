"""CPU model of the a2 ring of the CNN2D blocks 1-3 kernels (csrc/conv123_body.h) with the consumers' step barrier behind
fragment read DFA_C123_CBAR instead of read 4.  Both roles are walked interval by interval (an interval = the code between
two workgroup barriers); every a2 row carries a tag (unit, row) so that a read can be checked against the row it is meant
to see.  The model asserts that every read finds its row written in an EARLIER interval, that no row is overwritten in or
before the interval of its last read, and that the two roles execute the same number of barriers: for niter3 = 1 .. 48
and every CBAR = 0 .. 35.  CBAR = 36 must fail (read 36 is the first of a row the producers write in that interval), in the
model and in the header's static_assert.  conv123_phase.hip, the kernel built with CBAR = 35, is put through the static
LDS-pipeline check and the register budget."""
import os
import re
import subprocess

import pytest

from conv123_common import CSRC, _checker, _compiled, _pipelined_fit_two_waves_per_simd

SRC = os.path.join(CSRC, "conv123_carry.hip")
PHASE_SRC = os.path.join(CSRC, "conv123_phase.hip")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")

NR = 48            # fragment reads of a consumer iteration: 4 ring rows x 12
CBAR_MAX = 35


def _read_target(it, s):
    """fragment read s of consumer iteration it -> (ring block, ring row), a2 row"""
    i = s // 12
    return ((it + i // 2) & 3, i & 1), 2 * it - 1 + i


def _producer(n, units):
    """intervals of ("W", (block, row), tag): the a2 hand-off of producer iteration it follows its MFMA stream, i.e. barrier
    #it, and is complete before the role reaches #(it + 1) (in-order LDS, counted wait in front of that barrier)"""
    prog, cur = [], []

    def bar():
        nonlocal cur
        prog.append(cur)
        cur = []

    bar(); bar(); bar(); bar()                                           # prologue of the first unit
    for v in range(units):
        for it in range(n):
            bar()                                                        # #it
            cur.append(("W", (it & 3, 1), (v, 2 * it)))                  # a2 row 2 it      -> block it, row 1
            cur.append(("W", ((it + 1) & 3, 0), (v, 2 * it + 1)))        # a2 row 2 it + 1  -> block it + 1, row 0
        cur.append(("W", (n & 3, 1), (v, 2 * n)))                        # the zero row 2 niter3
        if v + 1 < units:
            bar(); bar(); bar()                                          # T1, T2, N1
        else:
            bar(); bar()
    prog.append(cur)
    return prog


def _consumer(n, units, cbar):
    prog, cur = [], []

    def bar():
        nonlocal cur
        prog.append(cur)
        cur = []

    cur.append(("W", (0, 0), (0, -1)))                                   # ring row -1 of the first unit
    bar(); bar(); bar(); bar()
    for v in range(units):
        bar(); bar()                                                     # idle steps: #0, #1
        for it in range(n):
            for s in range(NR):
                loc, row = _read_target(it, s)
                cur.append(("R", loc, (v, row)))
                if s == cbar:
                    bar()                                                # #(it + 2)
            if cbar >= NR:
                bar()
        if v + 1 < units:
            bar()                                                        # N1
            cur.append(("W", (0, 0), (v + 1, -1)))
    prog.append(cur)
    return prog


def _walk(n, units, cbar):
    """returns the list of findings (empty = sound)"""
    prod, cons = _producer(n, units), _consumer(n, units, cbar)
    if len(prod) != len(cons):
        return [("barrier counts differ", len(prod) - 1, len(cons) - 1)]
    bad, mem = [], {}
    for k, (p, c) in enumerate(zip(prod, cons)):
        written = {}
        for role, ops in (("producers", p), ("consumers", c)):
            for a, loc, tag in ops:
                if a == "W":
                    if loc in written:
                        bad.append((k, "two writes of one row in one interval", loc, written[loc], tag))
                    written[loc] = tag
        for a, loc, tag in c:
            if a != "R":
                continue
            if loc in written:        # all four consumer waves read every row: a write in the same interval is a race
                bad.append((k, "read and write of one row in one interval", loc, tag, written[loc]))
            elif mem.get(loc) != tag:
                bad.append((k, "read does not see its row", loc, tag, mem.get(loc)))
        mem.update(written)
    return bad


@pytest.mark.parametrize("n", range(1, 49))
def test_phase123_a2_ring_model(n):
    for cbar in range(0, CBAR_MAX + 1):
        for units in (1, 2, 3):
            bad = _walk(n, units, cbar)
            assert not bad, (n, cbar, units, bad[:3])


@pytest.mark.parametrize("n", [2, 3, 4, 5, 7, 40, 48])
def test_phase123_model_rejects_cbar_36(n):
    """Read 36 is the first read of block it + 1, row 1 = a2 row 2 it + 2, which the producers write in the very interval
    that ends at the consumers' barrier: with the barrier behind it the read races with the write.  (niter3 = 1 has no
    such row: its row 2 is the zero row, written one interval earlier.)"""
    bad = _walk(n, 2, CBAR_MAX + 1)
    assert bad and all(b[1] == "read and write of one row in one interval" for b in bad), bad[:3]
    rows = {b[3][1] for b in bad}
    assert rows <= {2 * it + 2 for it in range(n)}, rows


def test_phase123_model_catches_a_consumer_one_step_early():
    """Not vacuous the other way either: consumers that skip an idle step read rows nobody has written yet."""
    n, cbar = 12, 28
    prod, cons = _producer(n, 1), _consumer(n, 1, cbar)
    early = cons[:4] + [cons[4] + cons[5]] + cons[6:]
    assert len(early) == len(prod) - 1
    mem, bad = {}, []
    for p, c in zip(prod, early):
        written = {loc: tag for a, loc, tag in p + c if a == "W"}
        bad += [tag for a, loc, tag in c if a == "R" and (loc in written or mem.get(loc) != tag)]
        mem.update(written)
    assert bad


# ------------------------------------------------------------------------------------------------------ the macro itself
def _hipcc():
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    return HIPCC


@pytest.mark.parametrize("cbar,ok", [(35, True), (36, False), (-1, False)])
def test_phase123_header_refuses_a_barrier_behind_read_35(cbar, ok):
    out = subprocess.run([_hipcc(), "-std=c++17", "--offload-arch=gfx950", "--offload-device-only", "-fsyntax-only",
                          "-DDFA_C123_CBAR=(%d)" % cbar, SRC], capture_output=True, text=True, cwd=CSRC)
    assert (out.returncode == 0) == ok, out.stderr[-2000:]
    if not ok:
        assert "static assertion failed" in out.stderr and "S_BAR" in out.stderr, out.stderr[-2000:]


def test_phase123_static_check_and_registers():
    """conv123_phase.hip (barrier behind read 35, consumers at priority 1): four kernels, counted waits and operand
    provenance hold, <= 256 VGPRs (arch + acc) and no scratch in the two pipelined kernels.  The position moves no LDS
    operation, only the barrier between them."""
    chk, (asm, usage) = _checker(), _compiled(PHASE_SRC)
    kernels, nreads, violations = chk.check_asm(asm)
    assert kernels == 4 and nreads > 0 and not violations, violations[:5]
    nk, nm, v2 = chk.check_operand_provenance(asm)
    assert nm > 0 and not v2, v2[:5]
    assert asm.count("s_setprio 1") >= 4 and "conv123_carry_kernel" not in asm      # its own kernels, the consumers raised
    _pipelined_fit_two_waves_per_simd(usage, "conv123_phase_kernel")


def test_phase123_file_sets_the_last_legal_position():
    text = open(PHASE_SRC).read()
    assert re.search(r"^#define DFA_C123_CBAR 35$", text, re.M) and re.search(r"^#define DFA_C123_PRIO 1$", text, re.M)
    assert re.search(r"^#define DFA_C123_CARRY 1$", text, re.M)
    # ... and its LDS bytes are the carry form's, side buffer included: both files launch through c123_launch as DFA_CONV123_CARRY,
    # which takes grid and bytes from conv123_plan, and neither sizes or launches anything itself
    for t in (text, open(SRC).read()):
        assert re.search(r"return c123_launch\(DFA_C123_KERNEL\(conv123_\w+_kernel, x_dtype, pipe\), DFA_CONV123_CARRY, ", t)
        assert "hipLaunchKernelGGL" not in t and "MaxDynamicSharedMemorySize" not in t
