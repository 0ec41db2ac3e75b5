"""CPU checks of conv123_persist.hip (CNN2D blocks 1-3, one persistent workgroup per CU): the static LDS-pipeline check of
the compiled gfx950 assembly, the register budget (two waves per SIMD, no scratch), the range assignment, and a host model
of the schedule across the boundary between two units of a workgroup."""
import os
import re

import pytest

from conv123_common import CSRC, _checker, _compiled, _pipelined_fit_two_waves_per_simd

SRC = os.path.join(CSRC, "conv123_persist.hip")


def test_persist123_lds_pipeline_static_check():
    chk, asm = _checker(), _compiled(SRC)[0]
    kernels, nreads, violations = chk.check_asm(asm)
    assert not violations, violations[:5]
    assert nreads > 0
    nk, nm, v2 = chk.check_operand_provenance(asm)
    assert nm > 0 and not v2, v2[:5]


def test_persist123_registers_fit_two_waves_per_simd():
    """512 threads, one workgroup per CU: <= 256 VGPRs per wave (arch + acc) and no scratch in the pipelined kernels.
    (The compiler-scheduled twins are a test hook: they may spill a little.)"""
    _pipelined_fit_two_waves_per_simd(_compiled(SRC)[1], "conv123_persist_kernel")     # its own kernels, under its own name


def _ranges(nunits, nwg):
    """The kernel's assignment: blockIdx -> (xcd, index) -> logical workgroup -> [u0, u1)."""
    out = []
    xq, xr = nwg >> 3, nwg & 7
    uq, urem = nunits // nwg, nunits % nwg
    for bid in range(nwg):
        xcd, xi = bid & 7, bid >> 3
        lw = (xcd * (xq + 1) if xcd < xr else xr * (xq + 1) + (xcd - xr) * xq) + xi
        u0 = lw * uq + min(lw, urem)
        out.append((lw, u0, u0 + uq + (1 if lw < urem else 0)))
    return out


@pytest.mark.parametrize("nunits,nwg", [(1536, 256), (1200, 256), (516, 256), (512, 256), (576, 304), (513, 512), (7, 7), (1000, 13)])
def test_persist123_ranges_partition_the_units(nunits, nwg):
    rs = _ranges(nunits, nwg)
    assert sorted(lw for lw, _, _ in rs) == list(range(nwg))                  # the remap is a permutation of the workgroups
    spans = sorted((u0, u1) for _, u0, u1 in rs)
    assert spans[0][0] == 0 and spans[-1][1] == nunits
    assert all(a[1] == b[0] for a, b in zip(spans, spans[1:]))                # contiguous, disjoint, complete
    sizes = {u1 - u0 for u0, u1 in spans}
    assert min(sizes) >= 1 and max(sizes) - min(sizes) <= 1
    if nwg % 8 == 0:                                                          # neighbouring ranges on one XCD (blockIdx & 7)
        by_lw = {lw: bid & 7 for bid, (lw, _, _) in enumerate(rs)}
        per = nwg // 8
        assert all(by_lw[lw] == lw // per for lw in range(nwg))


# ---------------------------------------------------------------------------------------------------- boundary schedule
# A role's program as a list of barrier intervals; an interval is a list of (access, resource) with access "R" or "W".
# Resources: ("win", buf) feature-window buffer; ("a1", blk) a1 ring block; ("a2", blk, row) a row of the consumers' ring;
# ("tot",) the consumers' running totals (lane-private, listed so that read-out-before-zero shows in the model).
# Every resource but ("tot",) is read by all waves of the reading role, so a write and a read of it in one interval are a race
# whichever roles they come from; two writes by different roles are one too.

def _producer(n, units):
    prog, cur = [], []

    def bar():
        nonlocal cur
        prog.append(cur)
        cur = []

    def produce(j, blk):
        cur.extend([("R", ("win", j & 1)), ("W", ("a1", blk))])

    # first unit: the four-barrier prologue
    bar()                                                    # pads / biases / (consumers: ring row -1)
    cur.extend([("W", ("win", 0)), ("W", ("win", 1))])       # x_store(0), x_store(1)
    bar()
    produce(0, 0); produce(1, 1)
    bar()
    cur.append(("W", ("win", 0)))                            # feature block 2
    bar()
    for v in range(units):
        for it in range(n):
            ph = it % 3
            cur.append(("R", ("a1", ph)))                    # fragment reads 0 .. S_BAR: ring rows of block ph
            bar()                                            # the step's barrier
            cur.extend([("R", ("a1", ph)), ("R", ("a1", (ph + 1) % 3))])
            cur.append(("R", ("win", (it + 2) & 1)))         # c1_issue(it + 2)
            cur.append(("W", ("a1", (ph + 2) % 3)))          # c1_store
            cur.append(("W", ("win", (it + 3) & 1)))         # x_store((it + 3) & 1)
            cur.append(("W", ("a2", it & 3, 1)))             # a2 row 2 it      (row pair 0)
            cur.append(("W", ("a2", (it + 1) & 3, 0)))       # a2 row 2 it + 1  (row pair 1)
        cur.append(("W", ("a2", n & 3, 1)))                  # zero row 2 n
        if v + 1 < units:                                    # unit boundary
            bar()                                            # T1
            cur.extend([("W", ("win", 0)), ("W", ("win", 1))])
            bar()                                            # T2
            produce(0, 0); produce(1, 1)
            bar()                                            # N1
            cur.append(("W", ("win", 0)))
        else:
            bar()
            bar()
    prog.append(cur)
    return prog


def _consumer(n, units, chunk):
    prog, cur = [], []

    def bar():
        nonlocal cur
        prog.append(cur)
        cur = []

    cur.extend([("W", ("a2", 0, 0)), ("W", ("tot",))])        # ring row -1, totals
    bar(); bar(); bar(); bar()
    for v in range(units):
        bar(); bar()                                         # idle steps 0, 1
        for it in range(n):
            ph = it & 3
            cur.append(("R", ("a2", ph, 0)))                 # fragment reads 0 .. S_BAR
            bar()
            cur.extend([("R", ("a2", ph, 0)), ("R", ("a2", ph, 1)), ("R", ("a2", (ph + 1) & 3, 0)), ("R", ("a2", (ph + 1) & 3, 1))])
            if (it + 1) % chunk == 0 or it + 1 == n:
                cur.extend([("R", ("tot",)), ("W", ("tot",))])
        if v + 1 < units:
            bar()                                            # N1
            cur.append(("W", ("a2", 0, 0)))                  # row -1 of the next unit
        cur.append(("R", ("tot",)))                          # time mean -> emb
        if v + 1 < units:
            cur.append(("W", ("tot",)))
    prog.append(cur)
    return prog


def _races(prod, cons):
    bad = []
    for i, (p, c) in enumerate(zip(prod, cons)):
        pw = {r for a, r in p if a == "W"}
        pr = {r for a, r in p if a == "R"}
        cw = {r for a, r in c if a == "W"}
        cr = {r for a, r in c if a == "R"}
        for res in (pw & cr) | (cw & pr) | (pw & cw):
            bad.append((i, "roles", res))
        for res in ((pw & pr) | (cw & cr)) - {("tot",)}:      # one role, but all of its waves read what each wave writes
            bad.append((i, "waves", res))
    return bad


@pytest.mark.parametrize("n", range(5, 49))
def test_persist123_boundary_schedule_model(n):
    chunk = 12
    for units in (1, 2, 3):
        prod, cons = _producer(n, units), _consumer(n, units, chunk)
        # barriers = intervals - 1: equal in both roles, n + 6 for the first unit of a workgroup, n + 3 for each later one
        assert len(prod) == len(cons) == 1 + (n + 6) + (units - 1) * (n + 3), (n, units, len(prod), len(cons))
        assert not _races(prod, cons), (n, units, _races(prod, cons)[:4])
    # the totals: zeroed, then (add = read + write)*, read out, zeroed, ... and read out last -- never zeroed unread
    order = "".join(a for iv in _consumer(n, 3, chunk) for a, r in iv if r == ("tot",))
    assert re.fullmatch(r"W(RW)*R", order), order


def test_persist123_model_catches_a_missing_boundary_barrier():
    """The model is not vacuous: without N1 the consumers' last reads meet the zeroing of row -1 (for niter3 = 0 mod 4 etc.),
    and without T1 the window stores meet the last c1_issue."""
    n = 40
    prod, cons = _producer(n, 2), _consumer(n, 2, 12)
    first = 1 + (n + 6)                                      # intervals of the first unit
    merged_p = prod[:first - 3] + [prod[first - 3] + prod[first - 2]] + prod[first - 1:]      # no T1 in the producers
    assert len(merged_p) != len(cons) and any(b[2][0] == "win" for b in _races(merged_p, cons))
    merged_c = cons[:first - 1] + [cons[first - 1] + cons[first]] + cons[first + 1:]          # no N1 in the consumers
    assert len(merged_c) != len(prod) and ((first - 1, "waves", ("a2", 0, 0)) in _races(prod, merged_c))
