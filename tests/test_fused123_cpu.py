"""CPU checks of conv123_fused.hip (CNN2D blocks 1-3 in one kernel): the static LDS-pipeline check of the compiled gfx950
assembly, the register budget of two waves per SIMD without scratch, and the LDS bank model of the producers' a2 hand-off."""
import os

from conv123_common import CSRC, _checker, _compiled, _pipelined_fit_two_waves_per_simd

SRC = os.path.join(CSRC, "conv123_fused.hip")


def test_fused123_lds_pipeline_static_check():
    chk, asm = _checker(), _compiled(SRC)[0]
    kernels, nreads, violations = chk.check_asm(asm)
    assert not violations, violations[:5]
    assert nreads > 0
    nk, nm, v2 = chk.check_operand_provenance(asm)
    assert nm > 0 and not v2, v2[:5]


def test_fused123_registers_fit_two_waves_per_simd():
    """512 threads, one workgroup per CU: <= 256 VGPRs per wave (arch + acc) and no scratch in the pipelined kernels.
    (The compiler-scheduled twins are a test hook: they may spill a little.)"""
    _pipelined_fit_two_waves_per_simd(_compiled(SRC)[1], "conv123_fused_kernel")


def test_fused123_a2_handoff_bank_model():
    """The producers write a pooled a2 row with ds_write_b128 into block 3's layout: lane (r = lane & 31, h = lane >> 5)
    stores chunk c = 4 nsl + h + 2 g of pixel slot r at r * 128 + ((c ^ (r & 6)) << 4).  In the 16-lane groups gfx950 services
    a b128 access in, the 16 stores fall in 8 distinct bank quads: a 2-way conflict, 2 stores per lane and iteration against
    the consumers' 48 conflict-free fragment reads (test_host_api.py::test_m16_swizzle_is_conflict_free)."""
    groups = [list(range(0, 4)) + list(range(12, 16)) + list(range(20, 28)),
              list(range(4, 12)) + list(range(16, 20)) + list(range(28, 32)),
              list(range(32, 36)) + list(range(44, 48)) + list(range(52, 60)),
              list(range(36, 44)) + list(range(48, 52)) + list(range(60, 64))]
    for nsl in range(2):
        for g in range(2):
            for grp in groups:
                quads = set()
                for lane in grp:
                    r, h = lane & 31, lane >> 5
                    c = 4 * nsl + h + 2 * g
                    quads.add(((r * 128 + ((c ^ (r & 6)) << 4)) // 16) % 16)
                assert len(quads) == 8, (nsl, g)
    # every (slot, chunk) of a ring row is written exactly once per row by the four producer waves of a row pair
    seen = set()
    for nsl in range(2):
        for g in range(2):
            for lane in range(64):
                r, h = lane & 31, lane >> 5
                c = 4 * nsl + h + 2 * g
                seen.add(r * 128 + ((c ^ (r & 6)) << 4))
    assert seen == set(range(0, 32 * 128, 16))
