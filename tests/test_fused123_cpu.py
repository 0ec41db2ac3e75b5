"""CPU checks of conv123_fused.hip (CNN2D blocks 1-3 in one kernel): the static LDS-pipeline check of the compiled gfx950
assembly, the register budget of two waves per SIMD without scratch, and the LDS bank model of the producers' a2 hand-off."""
import importlib.util
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "deep-fake-audio-classifier_amd", "csrc", "conv123_fused.hip")


def _checker():
    spec = importlib.util.spec_from_file_location("check_lds_pipeline", os.path.join(ROOT, "tools", "check_lds_pipeline.py"))
    chk = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(chk)
    if not os.path.exists(chk.HIPCC):
        pytest.skip("hipcc not available")
    return chk


def test_fused123_lds_pipeline_static_check():
    chk = _checker()
    asm = chk.compile_to_asm(SRC)
    kernels, nreads, violations = chk.check_asm(asm)
    assert not violations, violations[:5]
    assert nreads > 0
    nk, nm, v2 = chk.check_operand_provenance(asm)
    assert nm > 0 and not v2, v2[:5]


def test_fused123_registers_fit_two_waves_per_simd(tmp_path):
    """512 threads, one workgroup per CU: <= 256 VGPRs per wave (arch + acc) and no scratch in the pipelined kernels.
    (The compiler-scheduled twins are a test hook: they may spill a little.)"""
    chk = _checker()
    out = subprocess.run([chk.HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "--offload-device-only", "-c", SRC,
                          "-o", str(tmp_path / "k.o"), "-Rpass-analysis=kernel-resource-usage"],
                         capture_output=True, text=True, cwd=os.path.dirname(SRC))
    assert out.returncode == 0, out.stderr[-2000:]
    usage, name = {}, None
    for line in out.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            usage[name] = {}
            continue
        m = re.search(r"remark:\s+(VGPRs|AGPRs|ScratchSize \[bytes/lane\]): (\d+)", line)
        if m and name:
            usage[name][m.group(1)] = int(m.group(2))
    piped = {k: v for k, v in usage.items() if "conv123_fused_kernel" in k and "Lb1E" in k}
    assert len(piped) == 2, usage
    for k, v in piped.items():
        assert v["VGPRs"] + v["AGPRs"] <= 256, (k, v)
        assert v["ScratchSize [bytes/lane]"] == 0, (k, v)


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
