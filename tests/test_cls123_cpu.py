"""CPU model of the barrier sequences of conv123_cls.hip (csrc/conv123_body.h with DFA_C123_LATE_EMIT and DFA_C123_CLS; the
shipped file sets CLS alone -- the late EMIT was measured and left out, it stays a build option and its model stays here): the
phase form whose consumers store a unit's time mean between the two idle barriers of the NEXT unit and, behind the last unit,
compute the classifier head of the workgroup's utterances.  Both roles are written down as the event lists the code executes,
one list per interval (an interval = the code between two workgroup barriers), for niter3 = 1 .. 48 and ranges of 1, 2, 3 and 6
units.  The model asserts that both roles execute the same number of barriers, the trailing classifier barriers included; that
EMIT of unit u falls between idle barriers 0 and 1 of unit u + 1 (the last unit's behind its last iteration); that ring row -1
is zeroed before idle barrier 0 of its unit and is neither read nor written by the producers before; and that `tot` is zeroed
before iteration 0.  The file is put through the static LDS-pipeline check and the register budget, and the checker's new rule
(a backward branch taken with reads in flight is followed) is shown to catch what it must."""
import os
import re

import pytest

from conv123_common import CSRC, _checker, _compiled, _pipelined_fit_two_waves_per_simd

CLS_SRC = os.path.join(CSRC, "conv123_cls.hip")
BODY = os.path.join(CSRC, "conv123_body.h")


def _producer(n, units, nstrips):
    """c123_producer, PERSIST + CLS: intervals of events"""
    prog, cur = [], []

    def bar(name):
        nonlocal cur
        prog.append((name, cur))
        cur = []

    for k in range(4):
        bar("prologue")
    for v in range(units):
        for it in range(n):
            bar(("step", v, it))                       # the barrier stands in front of the step's MFMA stream
            cur.append(("a2", v, 2 * it))
            cur.append(("a2", v, 2 * it + 1))
        cur.append(("a2", v, 2 * n))                   # the zero row
        if v + 1 < units:
            bar(("T1", v)); bar(("T2", v)); bar(("N1", v))
        else:
            bar(("idle", v)); bar(("idle", v))
    for k in range(units // nstrips + 1):              # the consumers' classifier barriers
        bar("cls")
    prog.append(("end", cur))
    return prog


def _consumer(n, units, nstrips):
    """c123_consumer, PERSIST + LATE_EMIT + CLS"""
    prog, cur = [], []

    def bar(name):
        nonlocal cur
        prog.append((name, cur))
        cur = []

    cur.append(("zero_row", 0))
    cur.append(("zero_tot", 0))
    for k in range(4):
        bar("prologue")
    u = 0
    while True:
        bar(("idle0", u))
        if u != 0:
            cur.append(("emit", u - 1))
            cur.append(("zero_tot", u))
        bar(("idle1", u))
        for it in range(n):
            cur.append(("reads", u, it, "early"))      # reads 0 .. 35
            bar(("cstep", u, it))
            cur.append(("reads", u, it, "late"))       # reads 36 .. 47, then the flush into tot
            cur.append(("flush", u, it))
        last = u + 1 >= units
        if not last:
            bar(("N1", u))
            cur.append(("zero_row", u + 1))
            u += 1
            continue
        cur.append(("emit", u))
        break
    bar("cls")                                         # behind the release of the last EMIT's stores
    for k in range(units // nstrips):
        cur.append(("dot", k))
        cur.append(("part", k & 1, k))
        bar("cls")
        cur.append(("logit", k & 1, k))
    prog.append(("end", cur))
    return prog


def _where(prog, ev):
    hits = [i for i, (_, evs) in enumerate(prog) if ev in evs]
    assert len(hits) == 1, (ev, hits)
    return hits[0]


def _bar_index(prog, name):
    hits = [i for i, (nm, _) in enumerate(prog) if nm == name]
    assert len(hits) == 1, (name, hits)
    return hits[0]         # the barrier that ENDS interval i; interval i + 1 follows it


RANGES = [(1, 1), (2, 1), (2, 2), (3, 1), (3, 3), (6, 1), (6, 2), (6, 3), (6, 6)]     # (units, strips per utterance)


@pytest.mark.parametrize("n", range(1, 49))
def test_cls123_barrier_model(n):
    for units, nstrips in RANGES:
        prod, cons = _producer(n, units, nstrips), _consumer(n, units, nstrips)
        assert len(prod) == len(cons), (n, units, nstrips, len(prod) - 1, len(cons) - 1)
        assert len(prod) - 1 == 4 + units * (n + 2) + (units - 1) + 1 + units // nstrips
        # the roles' barriers pair up as the kernel means them to: consumer idle barrier 0 of unit u is the producers' step 0
        for u in range(units):
            assert _bar_index(cons, ("idle0", u)) == _bar_index(prod, ("step", u, 0))
            if n > 1:
                assert _bar_index(cons, ("idle1", u)) == _bar_index(prod, ("step", u, 1))
            for it in range(n):
                if it + 2 < n:
                    assert _bar_index(cons, ("cstep", u, it)) == _bar_index(prod, ("step", u, it + 2))
            if u + 1 < units:
                assert _bar_index(cons, ("N1", u)) == _bar_index(prod, ("N1", u))
        for u in range(units):
            e = _where(cons, ("emit", u))
            if u + 1 < units:      # between idle barriers 0 and 1 of unit u + 1: under the producers' step 0
                assert _bar_index(cons, ("idle0", u + 1)) < e <= _bar_index(cons, ("idle1", u + 1)), (n, units, u)
                assert e == _bar_index(prod, ("step", u + 1, 0)) + 1
            else:                  # the last unit: behind its last iteration, in front of the first classifier barrier
                assert e == _where(cons, ("flush", u, n - 1))
                assert cons[e][0] == "cls"
            # tot: zeroed behind the EMIT that read it and before iteration 0 of the next unit (whose first flush follows)
            z = _where(cons, ("zero_tot", u))
            assert z < _where(cons, ("flush", u, 0)) and z <= _bar_index(cons, ("idle1", u))
            if u > 0:
                assert cons[z][1].index(("emit", u - 1)) < cons[z][1].index(("zero_tot", u))
                assert _where(cons, ("flush", u - 1, n - 1)) < z
            # ring row -1: zeroed before idle barrier 0 of its unit, i.e. before the interval of the producers' first a2 write of the
            # unit (behind their step-0 barrier), behind the consumers' last read of the unit before, two barriers before its reader
            zr = _where(cons, ("zero_row", u))
            assert zr <= _bar_index(cons, ("idle0", u))
            assert zr < _where(prod, ("a2", u, 0))
            assert zr + 2 <= _where(cons, ("reads", u, 0, "early"))
            if u > 0:
                assert zr > _where(cons, ("reads", u - 1, n - 1, "late"))
        # classifier: every dot product behind the barrier that follows the last EMIT; part words of one parity are rewritten only
        # after the barrier thread 0 reaches behind its read of them
        first_cls = _where(cons, ("emit", units - 1))
        for k in range(units // nstrips):
            assert _where(cons, ("dot", k)) > first_cls
            assert _where(cons, ("logit", k & 1, k)) == _where(cons, ("part", k & 1, k)) + 1
            if k >= 2:
                assert _where(cons, ("part", k & 1, k)) > _where(cons, ("logit", k & 1, k - 2))


def test_cls123_model_catches_a_missing_trailing_barrier():
    """not vacuous: producers that return behind their last idle step leave the consumers one short per utterance and one"""
    prod, cons = _producer(5, 6, 3), _consumer(5, 6, 3)
    assert len(prod) == len(cons)
    assert len([p for p in prod if p[0] != "cls"]) == len(cons) - (6 // 3 + 1)


def test_cls123_file_sets_the_macros():
    text, body = open(CLS_SRC).read(), open(BODY).read()
    for name, val in (("DFA_C123_CARRY", 1), ("DFA_C123_CBAR", 35), ("DFA_C123_PRIO", 1)):
        assert re.search(r"^#define %s %d$" % (name, val), text, re.M), name
    assert re.search(r"^#ifndef DFA_C123_CLS\n#define DFA_C123_CLS 1\n#endif$", text, re.M)
    assert re.search(r"^#ifndef DFA_C123_LATE_EMIT\n#define DFA_C123_LATE_EMIT 0 ", text, re.M)      # tried, measured, left out
    for name in ("DFA_C123_LATE_EMIT", "DFA_C123_CLS"):
        assert re.search(r"^#ifndef %s\n#define %s 0\n#endif$" % (name, name), body, re.M), name     # off in the four older kernels
    assert re.search(r"return c123_launch\(DFA_C123_KERNEL\(conv123_cls_kernel, x_dtype, pipe\), DFA_CONV123_CARRY, ", text)
    assert "hipLaunchKernelGGL" not in text and "MaxDynamicSharedMemorySize" not in text
    # the producers' trailing barriers and the consumers' are counted by the same expression: one, then one per utterance
    assert "for (int k = (u_end - cls_u0) / a.nstrips; k >= 0; --k) __syncthreads();" in body
    assert "c123_classifier(a, smem, nsl, u_first / a.nstrips, u_end / a.nstrips);" in body


def test_cls123_static_check_and_registers():
    """conv123_cls.hip: four kernels, counted waits and operand provenance hold, <= 256 VGPRs (arch + acc) and no scratch in the
    two pipelined kernels (the classifier's batched loads live in registers that are dead behind the last unit)."""
    chk, (asm, usage) = _checker(), _compiled(CLS_SRC)
    kernels, nreads, violations = chk.check_asm(asm)
    assert kernels == 4 and nreads > 0 and not violations, violations[:5]
    nk, nm, v2 = chk.check_operand_provenance(asm)
    assert nm > 0 and not v2, v2[:5]
    assert asm.count("s_setprio 1") >= 4 and "conv123_phase_kernel" not in asm
    _pipelined_fit_two_waves_per_simd(usage, "conv123_cls_kernel")


# ---------------------------------------------------------------------------------------- the checker's followed branches
_HEAD = "_Z1kv:\n"
_READ = ";;#ASMSTART\nds_read_b128 v[4:7], v1\n;;#ASMEND\n"


def _violations(body):
    return _checker().check_asm(_HEAD + body + "s_endpgm\n")[2]


def test_checker_follows_a_join_block_placed_above_its_branch():
    # the join block (.L1) waits for the read before it uses it: clean, although the branch to it goes backward
    ok = "s_branch .L2\n.L1:\ns_waitcnt lgkmcnt(0)\nv_mov_b32 v9, v4\ns_branch .L3\n.L2:\n" + _READ + "s_branch .L1\n.L3:\n"
    assert not _violations(ok)
    # ... and flagged where the join block uses the destination without a wait
    bad = "s_branch .L2\n.L1:\nv_mov_b32 v9, v4\ns_waitcnt lgkmcnt(0)\ns_branch .L3\n.L2:\n" + _READ + "s_branch .L1\n.L3:\n"
    v = _violations(bad)
    assert v and "touches an in-flight LDS destination" in v[0][2], v


def test_checker_still_refuses_a_read_carried_around_a_loop():
    loop = ".L1:\nv_add_u32 v2, v2, v3\n" + _READ + "s_cbranch_scc1 .L1\ns_waitcnt lgkmcnt(0)\n"
    v = _violations(loop)
    assert any("around a loop" in x[2] for x in v), v
