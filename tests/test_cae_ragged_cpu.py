"""CPU checks of the ragged auto-encoder score (dfa_cae_score_ragged): the C ABI exports and declarations, the planner, the
ragged kernel instantiations in the compiled gfx950 assembly (names, static LDS-pipeline rules, registers and scratch against
their uniform twins), the length validation, the argument check of the ragged ensemble CLIs, and an oracle control that
zero-padding is no substitute for the row masks."""
import importlib.util
import os
import re
import subprocess

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "deep-fake-audio-classifier_amd", "csrc")
CAE_RAGGED_SYMBOLS = ("dfa_cae_score_ragged", "dfa_cae_ragged_workspace_bytes")
# (source file, ragged kernel, its uniform twin, instantiations expected)
CAE_RAGGED_KERNELS = [("cae_enc1_mfma.hip", "cae_enc1_mfma_ragged_kernel", "cae_enc1_mfma_kernel", 2),
                      ("conv3x3_inst_cae.hip", "conv3x3_mfma_ragged_kernel", "conv3x3_mfma_kernel", 3),
                      ("cae_dec_fused.hip", "cae_dec_fused_ragged_kernel", "cae_dec_fused_kernel", 4),
                      ("cae.hip", "cae_mse_finalize_ragged_kernel", "cae_mse_finalize_kernel", 1)]


def _checker():
    spec = importlib.util.spec_from_file_location("check_lds_pipeline", os.path.join(ROOT, "tools", "check_lds_pipeline.py"))
    chk = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(chk)
    if not os.path.exists(chk.HIPCC):
        pytest.skip("hipcc not available")
    return chk


def test_cae_ragged_entry_points_exported_and_declared():
    header = open(os.path.join(ROOT, "include", "dfa_hip.h")).read()
    from dfa_amd import _lib
    lib = _lib.load()
    bound = {name for name, _, _ in _lib.SYMBOLS}
    for name in CAE_RAGGED_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert hasattr(lib, name), name
        assert name in bound, name


def test_cae_ragged_workspace_covers_the_uniform_plan():
    from dfa_amd import _lib
    lib = _lib.load()
    for B, T in ((1, 16), (32, 481), (256, 481), (7, 70)):
        uni = lib.dfa_workspace_bytes(None, _lib.MODEL_CAE, B, T, 180, _lib.PREC_BF16)
        rag = lib.dfa_cae_ragged_workspace_bytes(None, B, T, 180, _lib.PREC_BF16)
        assert uni > 0 and rag >= uni + 8 * B and rag % 256 == 0, (B, T, uni, rag)
    assert lib.dfa_cae_ragged_workspace_bytes(None, 0, 321, 180, _lib.PREC_BF16) == 0
    # the shared ragged planner keeps answering "no ragged forward" for the auto-encoder: callers test for that value
    assert lib.dfa_ragged_workspace_bytes(None, _lib.MODEL_CAE, 4, 321, 180, _lib.PREC_BF16) == 0


@pytest.fixture(scope="module")
def compiled(tmp_path_factory):
    """per source file: (assembly text, kernel-resource-usage remarks by mangled name)"""
    chk = _checker()
    cache = {}
    obj = str(tmp_path_factory.mktemp("cae_ragged") / "k.o")

    def get(src):
        if src not in cache:
            asm = chk.compile_to_asm(os.path.join(CSRC, src))
            flags = chk.per_file_flags(os.path.join(CSRC, src))
            out = subprocess.run([chk.HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "--offload-device-only", *flags, "-c", src,
                                  "-o", obj, "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True, cwd=CSRC)
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
            cache[src] = (asm, usage)
        return cache[src]
    return chk, get


@pytest.mark.parametrize("src,ragged,uniform,count", CAE_RAGGED_KERNELS)
def test_cae_ragged_kernels_exist_under_their_own_names(compiled, src, ragged, uniform, count):
    _, get = compiled
    asm, _ = get(src)
    names = set(re.findall(r"^(_Z\w+):", asm, re.M))
    rag = [n for n in names if ragged in n]
    assert len(rag) == count, sorted(names)
    assert not [n for n in rag if uniform in n]           # a function of its own name, not a template flag of the twin
    assert [n for n in names if uniform in n]


def test_cae_encoder_file_passes_the_lds_pipeline_check(compiled):
    """both static rules (in-flight destinations, matrix-operand provenance) with the ragged instantiations in the file"""
    chk, get = compiled
    asm, _ = get("conv3x3_inst_cae.hip")
    kernels, nreads, violations = chk.check_asm(asm)
    assert not violations, violations[:5]
    assert nreads > 0
    nk, nm, v2 = chk.check_operand_provenance(asm)
    # (the file keeps ONE diagnostic fp32 instantiation as the provenance rule's positive control, never launched by default:
    #  tests/test_host_api.py excludes it by the same name; nothing else may be flagged, and no ragged kernel)
    known = "conv3x3_mfma_kernelIfLi64ELi4ELi1ELi1ELi1ELi1ELi1ELb1ELb0ELb0ELi3E"
    others = [v for v in v2 if known not in v[0]]
    assert nm > 0 and not others, others[:5]
    assert not [v for v in v2 if "ragged" in v[0]]
    # the two asm-pipelined ragged instantiations (encoder blocks 2, 3) carry pipelined reads of their own
    for cin in ("Li32ELi2ELi2ELi2E", "Li64ELi4ELi1ELi1E"):
        m = re.search(r"^(_ZN3dfa26conv3x3_mfma_ragged_kernelINS_6bf16_tE%s\w+):(.*?)s_endpgm" % cin, asm, re.M | re.S)
        assert m and "ds_read_b128" in m.group(2) and ";#ASMSTART" in m.group(2), cin


def _twin(name, ragged, uniform):
    """mangled name of the uniform twin of a ragged instantiation: same template arguments"""
    m = re.match(r"_ZN3dfa\d+%s(I.*E)v" % ragged, name)
    return m.group(1) if m else ""


@pytest.mark.parametrize("src,ragged,uniform,count", CAE_RAGGED_KERNELS)
def test_cae_ragged_kernels_fit_the_register_budget_of_their_twins(compiled, src, ragged, uniform, count):
    """every ragged instantiation: no more VGPRs + AGPRs and no more scratch than the uniform instantiation with the same
    template arguments.  The finaliser (one thread per utterance, 8 waves per SIMD either way) is held to its final measured
    remark instead: its own tile count and divisor are two more per-lane values than the twin's scalar arguments, 10 VGPRs
    against 8 in each of the three forms tried."""
    _, get = compiled
    _, usage = get(src)
    rag = {k: v for k, v in usage.items() if ragged in k}
    assert len(rag) == count, sorted(usage)
    for k, v in rag.items():
        targs = _twin(k, ragged, uniform)
        twins = [u for u in usage if uniform in u and ragged not in u and (not targs or targs in u)]
        assert len(twins) == 1, (k, twins)
        t = usage[twins[0]]
        print(f"{k}: VGPRs {v['VGPRs']} AGPRs {v['AGPRs']} scratch {v['ScratchSize [bytes/lane]']}  |  twin: VGPRs {t['VGPRs']} "
              f"AGPRs {t['AGPRs']} scratch {t['ScratchSize [bytes/lane]']}")
        assert v["ScratchSize [bytes/lane]"] <= t["ScratchSize [bytes/lane]"], (k, v, t)
        budget = 10 if "finalize" in ragged else t["VGPRs"] + t["AGPRs"]
        assert v["VGPRs"] + v["AGPRs"] <= budget, (k, v, t)


@pytest.mark.parametrize("lengths,B,T_max,msg", [
    ([15, 40], 2, 40, r"lengths\[0\]=15"),         # too short for the four pools
    ([40, 41], 2, 40, r"lengths\[1\]=41"),         # T_max + 1
    ([40, 40, 40], 2, 40, r"3 lengths for a batch of 2"),
    ([16.0, 40.0], 2, 40, r"integers"),
    (torch.tensor([16.5, 40.0]), 2, 40, r"integers"),
])
def test_cae_score_rejects_bad_lengths_before_any_device_work(lengths, B, T_max, msg):
    """ConvAutoencoder.score(lengths=...) validates on the host first (no GPU here: a CPU tensor would raise RuntimeError later)"""
    from dfa_amd.model_cae import ConvAutoencoder
    m = ConvAutoencoder(precision="bf16").eval()
    with pytest.raises(ValueError, match=msg):
        m.score(torch.zeros(B, T_max, 180), lengths=lengths)


def test_cae_score_accepts_the_shortest_and_longest_length_on_the_host():
    from dfa_amd import _lib
    got = _lib.host_lengths([16, 40], 2, 40, 16)
    np.testing.assert_array_equal(got, np.array([16, 40], dtype=np.int32))


def test_ragged_member_check():
    from dfa_amd.hybrid_ensemble import check_ragged_members
    for members in (["cnn2d"], ["cae"], ["cnn2d", "cae"], ["cnn2d", "cnn1d", "cae"]):
        with pytest.raises(ValueError, match="--precision bf16 only"):
            check_ragged_members(members, "fp32")
        check_ragged_members(members, "bf16")
    with pytest.raises(ValueError, match="bf16 only"):
        check_ragged_members(["cnn2d", "cnn1d"], "bf16x3")
    for prec in ("fp32", "bf16", "bf16x3"):
        check_ragged_members(["cnn1d"], prec)
        check_ragged_members(["cnn1d", "cnn1d"], prec)
    with pytest.raises(ValueError, match="unknown ensemble member"):
        check_ragged_members(["mlp"], "bf16")


def test_is_ragged_looks_at_shapes_only():
    import pandas as pd
    from dfa_amd.hybrid_ensemble import is_ragged
    assert not is_ragged(pd.DataFrame({"features": [torch.zeros(180, 20), torch.ones(180, 20)]}))
    assert is_ragged(pd.DataFrame({"features": [torch.zeros(180, 20), torch.zeros(180, 21)]}))


@pytest.mark.parametrize("T", [17, 31, 47, 70])
def test_oracle_zero_padding_is_not_a_substitute_for_the_masks(golden, T):
    """Control (independent of the library): the score of a zero-padded utterance, taken over its own rows, is not the score
    of the utterance alone -- BatchNorm biases make the rows behind its end non-zero from block 1 on and the next convolution
    reads them.  With the oracle on the golden weights and this test's inputs: 5.5e-3, 2.3e-2, 1.7e-2, 4.5e-3 relative for
    T = 17, 31, 47, 70 (with other inputs 3.0e-3 at the least; 0 and 5e-6 for T = 16, 32: lengths that are multiples of 16
    hide a missing mask)."""
    from oracle import dfa_oracle as O
    sd, _ = golden("cae_eval")
    rng = np.random.default_rng(100 + T)
    x = rng.standard_normal((1, T, 180)).astype(np.float32)
    recon, _ = O.cae_forward(sd, x)
    alone = float(O.per_sample_mse(recon, x)[0])
    T_pad = 80
    xp = np.zeros((1, T_pad, 180), dtype=np.float32)
    xp[:, :T] = x
    rp, _ = O.cae_forward(sd, xp)
    padded = float(np.mean((rp[0, :T] - x[0]) ** 2))
    rel = abs(padded - alone) / alone
    print(f"T={T}: alone {alone:.6f} zero-padded {padded:.6f} relative difference {rel:.2e}")
    assert rel > 1e-3, (T, alone, padded, rel)
