"""What the tests of the CNN2D blocks 1-3 kernels (conv123_*.hip) share.  GPU side (tests/test_cnn2d_*123_gpu.py): the context,
the model, the features, a run under given options that checks which form the dispatcher took, and the fixture that puts the
options back.  CPU side (tests/test_*123_cpu.py): the loader of tools/check_lds_pipeline.py and the register budget of a form's
pipelined kernels.  A plain module, imported by name like ragged_train_oracle."""
import functools
import importlib.util
import os

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "deep-fake-audio-classifier_amd", "csrc")

PATTERNS = [0xFFFF, 0x7FC0, 0x7F80]
NONE, PER_UNIT, PERSIST, CARRY = 0, 1, 2, 3                  # DFA_CONV123_* (include/dfa_hip.h)
OPTS = ("fuse_blocks123", "persist123", "carry_a1", "lds_pipe", "phase123")


def _niter3(T):
    return (T // 2 // 2 + 1) // 2


def _ctx():
    from dfa_amd import _lib
    return _lib.Context.get(torch.device("cuda"))


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


@pytest.fixture(autouse=True)
def _restore_options():
    """Every option a blocks 1-3 test sets, back at its default.  Autouse in the test files that import it by name."""
    yield
    ctx = _ctx()
    for k in OPTS:
        ctx.set_option(k, 1)
    ctx.set_option("clock_probe", 0)


_MODELS = {}


def _model(F):
    if F not in _MODELS:
        from dfa_amd.model import CNN2D
        torch.manual_seed(5)
        m = CNN2D(in_features=F, precision="bf16").to("cuda")
        with torch.no_grad():
            for i in m._BN_IDX:
                m.conv[i].running_mean.normal_(0, 0.3)
                m.conv[i].running_var.uniform_(0.5, 2.0)
            m.classifier.weight.mul_(20.0)
        _MODELS[F] = m.eval()
    return _MODELS[F]


def _x(B, T, F, seed=11, dtype=torch.bfloat16, strided=True):
    gen = torch.Generator().manual_seed(seed)
    stored = torch.randn(B, F, T, generator=gen) * 3.2 - 0.07
    if strided:
        return stored.to("cuda").to(dtype).transpose(1, 2)          # [B, T, F] view of a [B, F, T] tensor
    return stored.transpose(1, 2).contiguous().to("cuda").to(dtype)


def _run(m, x, form=None, phase=None, **opts):
    """One forward with the given options, every other option of OPTS at 1; form / phase: what the dispatcher must report."""
    ctx = _ctx()
    for k in OPTS:
        ctx.set_option(k, opts.get(k, 1))
    lg, emb = m(x, return_embedding=True)
    torch.cuda.synchronize()
    if form is not None:
        assert ctx.last_conv123_form() == form, (ctx.last_conv123_form(), form, opts)
    if phase is not None:
        assert ctx.last_conv123_phase() == phase, (ctx.last_conv123_phase(), phase, opts)
    return lg.clone(), emb.clone()


def _same(got, want, what):
    assert torch.equal(got[0], want[0]), (what, "logits", (got[0] - want[0]).abs().max().item())
    assert torch.equal(got[1], want[1]), (what, "embeddings", (got[1] - want[1]).abs().max().item())


def _slots(m, x):
    ctx = _ctx()
    ctx.timing_reset()
    ctx.timing(True)
    m(x)
    torch.cuda.synchronize()
    ctx.timing(False)
    return [ctx.timing_read(s)[1] for s in range(4)]


def _probe_workgroups(m, x):
    ctx = _ctx()
    ctx.set_option("clock_probe", 1)
    m(x)
    torch.cuda.synchronize()
    n = ctx.clock_read()[3]
    ctx.set_option("clock_probe", 0)
    return n


# ------------------------------------------------------------------------------------------------------------ CPU side
def _checker():
    spec = importlib.util.spec_from_file_location("check_lds_pipeline", os.path.join(ROOT, "tools", "check_lds_pipeline.py"))
    chk = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(chk)
    if not os.path.exists(chk.HIPCC):
        pytest.skip("hipcc not available")
    return chk


@functools.lru_cache(maxsize=None)
def _compiled(src):
    """(assembly, resource usage per kernel) of a form's file as the library builds it: one compilation per file and session"""
    return _checker().resource_usage(src)


def _pipelined_fit_two_waves_per_simd(usage, kernel):
    """usage: _compiled(src)[1].  Every kernel in it is `kernel` (its own kernels, under its own name); the two
    pipelined ones (PIPE = true) hold <= 256 VGPRs per wave (arch + acc) and no scratch."""
    assert all(kernel in k for k in usage), list(usage)
    piped = {k: v for k, v in usage.items() if "Lb1E" in k}
    assert len(piped) == 2, usage
    for k, v in piped.items():
        assert v["VGPRs"] + v["AGPRs"] <= 256, (k, v)
        assert v["ScratchSize [bytes/lane]"] == 0, (k, v)
