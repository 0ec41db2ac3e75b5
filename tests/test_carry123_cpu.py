"""CPU checks of conv123_carry.hip (CNN2D blocks 1-3, persistent, two a1 columns carried from strip to strip): the static
LDS-pipeline and operand-provenance checks of the compiled gfx950 assembly, the register budget (two waves per SIMD, no
scratch), and a host model of the side buffer that holds the carried columns between two units of a workgroup."""
import os

import pytest

from conv123_common import CSRC, _checker, _compiled, _pipelined_fit_two_waves_per_simd

SRC = os.path.join(CSRC, "conv123_carry.hip")


def test_carry123_lds_pipeline_static_check():
    chk, asm = _checker(), _compiled(SRC)[0]
    kernels, nreads, violations = chk.check_asm(asm)
    assert kernels == 4 and not violations, violations[:5]
    assert nreads > 0
    nk, nm, v2 = chk.check_operand_provenance(asm)
    assert nm > 0 and not v2, v2[:5]


def test_carry123_registers_fit_two_waves_per_simd():
    """512 threads, one workgroup per CU: <= 256 VGPRs per wave (arch + acc) and no scratch in the two pipelined kernels.
    (The compiler-scheduled twins are a test hook: they may spill a little.)"""
    _pipelined_fit_two_waves_per_simd(_compiled(SRC)[1], "conv123_carry_kernel")       # its own kernels, under its own name


# ------------------------------------------------------------------------------------------------------ side buffer
# The side buffer as the kernel uses it.  A unit (utterance b, strip k) produces the a1 ring rows (j, m), j = 0 .. n + 1 ring
# blocks, m = 0 .. 3 rows = producer waves; LDS operations of one wave complete in its program order, and waves are not
# ordered against one another by anything the side buffer takes part in.  So a wave's program is a list of operations
#   ("load", entry)            the LDS read of an entry; its value goes to ring slots 0, 1 where the unit is not strip 0
#   ("store", entry, tag)      the lanes that hold slots 30, 31 write them over the entry; tag = (b, k, j, m)
#   ("ring01", j, m, k, use)   what the wave puts into ring slots 0, 1 of row (j, m): the value the load returned if `use`,
#                              else zeros (a select on the unit's strip number: the loaded value is dropped on strip 0)
# and the model runs the four programs in an arbitrary interleaving.

def _wave_program(m, n, utterances, strips, load_after_store=False, select_zero=True):
    prog = []
    for b in range(utterances):
        for k in range(strips):
            for j in range(n + 2):                 # produce_now(0), produce_now(1), then steps it = 0 .. n - 1 make block it + 2
                e = (j, m)
                load, store = ("load", e, (b, k)), ("store", e, (b, k, j, m))
                prog.extend([store, load] if load_after_store else [load, store])
                prog.append(("ring01", j, m, k, k > 0 or not select_zero))
    return prog


def _run_model(n, utterances, strips, order, load_after_store=False, select_zero=True):
    """order: the interleaving, a function (step) -> wave.  Returns the list of findings (empty = the carry is sound)."""
    progs = [_wave_program(m, n, utterances, strips, load_after_store, select_zero) for m in range(4)]
    pc = [0, 0, 0, 0]
    mem, writer, unread = {}, {}, {}             # entry -> tag of the last store / the wave that made it / not yet loaded
    loaded = [None] * 4
    bad, step = [], 0
    while any(pc[w] < len(progs[w]) for w in range(4)):
        w = order(step) % 4
        step += 1
        if pc[w] >= len(progs[w]):
            continue
        op = progs[w][pc[w]]
        pc[w] += 1
        if op[0] == "load":
            e, (b, k) = op[1], op[2]
            loaded[w] = mem.get(e, ("stale",))
            if k > 0:
                if e not in mem:
                    bad.append(("read before any write", e, b, k))
                elif writer[e] != w:
                    bad.append(("read by another wave than the writer", e, writer[e], w))
                unread[e] = False
        elif op[0] == "store":
            e, tag = op[1], op[2]
            b, k = tag[0], tag[1]
            if k > 0 and unread.get(e, False):
                bad.append(("overwritten before it was read", e, b, k))
            mem[e], writer[e], unread[e] = tag, w, True
        else:
            _, j, m, k, use = op
            t = loaded[w]
            if k == 0:
                if use:                          # stale LDS, or the last strip of the utterance before
                    bad.append(("strip 0 took an entry", (j, m), t))
            elif not use or t == ("stale",) or t[1:] != (k - 1, j, m):
                bad.append(("ring slots 0, 1 are not the previous strip's slots 30, 31", (j, m, k), t))
    return bad, mem


ORDERS = [
    lambda s: s,                       # round robin
    lambda s: s // 7,                  # bursts
    lambda s: (s * 2654435761) >> 7,   # scrambled
    lambda s: 3 - (s // 3) % 4,
]


@pytest.mark.parametrize("n", range(4, 49))
def test_carry123_side_buffer_model(n):
    for utterances in (1, 2, 3):
        for strips in (1, 2, 3, 6):
            for order in ORDERS[: 2 if n % 4 else 4]:
                bad, mem = _run_model(n, utterances, strips, order)
                assert not bad, (n, utterances, strips, bad[:3])
                # every entry of the n + 2 ring blocks is owned: written by its row's wave, last by the last unit of the range
                assert set(mem) == {(j, m) for j in range(n + 2) for m in range(4)}
                assert all(t[:2] == (utterances - 1, strips - 1) and t[2:] == e for e, t in mem.items())


def test_carry123_side_buffer_model_same_utterance():
    """The value a strip takes is its own utterance's: the tag that reaches ring slots 0, 1 carries utterance b."""
    progs_seen = []
    n, utterances, strips = 7, 3, 3
    prog = _wave_program(0, n, utterances, strips)
    mem, loaded = {}, None
    for op in prog:                              # one wave suffices: entries are per wave
        if op[0] == "load":
            loaded, cur = mem.get(op[1]), op[2]
        elif op[0] == "store":
            mem[op[1]] = op[2]
        elif op[3] > 0:
            progs_seen.append((cur[0], loaded[0]))
    assert progs_seen and all(b == src_b for b, src_b in progs_seen)


def test_carry123_model_catches_a_read_behind_the_write():
    """The model is not vacuous: with the load placed after the store a strip takes its OWN slots 30, 31."""
    bad, _ = _run_model(8, 2, 3, ORDERS[0], load_after_store=True)
    assert any(b[0] == "ring slots 0, 1 are not the previous strip's slots 30, 31" for b in bad), bad[:3]
    bad1, _ = _run_model(8, 1, 1, ORDERS[0], load_after_store=True)
    assert not bad1                              # (a one-strip utterance never uses an entry: nothing to catch)


def test_carry123_model_catches_a_missing_strip0_select():
    """Without the select the first strip of an utterance takes stale LDS (first unit of the workgroup) or the last strip
    of the utterance before it."""
    bad, _ = _run_model(8, 2, 3, ORDERS[0], select_zero=False)
    took = [b for b in bad if b[0] == "strip 0 took an entry"]
    assert any(b[2] == ("stale",) for b in took) and any(b[2] != ("stale",) and b[2][0] == 0 for b in took), bad[:3]
