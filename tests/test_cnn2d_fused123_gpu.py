"""CNN2D bf16 eval forward: blocks 1-3 + time mean in one kernel (conv123_fused.hip, context option "fuse_blocks123").
The fused path must reproduce the two-kernel path (conv12_fused + conv3_m16) bit for bit -- logits and embeddings -- wherever
the dispatcher takes it, its compiler-scheduled twin must equal the pipelined build, and stale LDS must not matter."""
import pytest
import torch

from conv123_common import PATTERNS, _ctx, _model, _restore_options, _run, _slots, _x  # noqa: F401 (_restore_options: autouse)

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("B,T,F,dtype,strided", [
    (256, 321, 180, torch.bfloat16, True),      # the headline
    (200, 321, 180, torch.bfloat16, True),
    (256, 321, 47, torch.bfloat16, True),       # ragged last strip
    (192, 321, 65, torch.bfloat16, True),
    (256, 322, 180, torch.bfloat16, True),      # odd H1 / H2 splits
    (256, 33, 180, torch.bfloat16, True),       # short T
    (256, 321, 180, torch.bfloat16, False),     # contiguous [B, T, F]
    (256, 321, 180, torch.float32, True),       # fp32 features, rounded to bf16 on load
])
def test_fused123_bit_identical_to_two_kernel_path(B, T, F, dtype, strided):
    m = _model(F)
    x = _x(B, T, F, dtype=dtype, strided=strided)
    want = _run(m, x, fuse_blocks123=0)
    got = _run(m, x, fuse_blocks123=1)
    assert torch.isfinite(got[0]).all()
    assert torch.equal(got[0], want[0]), (B, T, F, (got[0] - want[0]).abs().max().item())
    assert torch.equal(got[1], want[1]), (B, T, F, (got[1] - want[1]).abs().max().item())


def test_fused123_compiler_scheduled_twin():
    m = _model(180)
    x = _x(256, 321, 180)
    want = _run(m, x, fuse_blocks123=1, lds_pipe=1)
    got = _run(m, x, fuse_blocks123=1, lds_pipe=0)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])


def test_fused123_ignores_stale_lds():
    m = _model(47)
    x = _x(256, 321, 47)
    want = _run(m, x, fuse_blocks123=1)
    for pat in PATTERNS:
        _ctx().set_option("poison_lds", pat)
        got = _run(m, x)
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), hex(pat)


def test_fused123_dispatch():
    m = _model(180)
    assert _slots(m, _x(256, 321, 180)) == [0, 0, 1, 1]        # one fused kernel (slot 2) + the classifier (slot 3)
    assert _slots(m, _x(8, 321, 180)) == [0, 1, 1, 1]          # small batch: the time-split two-kernel path
    _ctx().set_option("fuse_blocks123", 0)
    assert _slots(m, _x(256, 321, 180)) == [0, 1, 1, 1]


def test_fused123_batch_independence():
    """An utterance alone (time-split two-kernel path) gives the logit it gets inside a batch of 256 (fused path)."""
    m = _model(180)
    x = _x(256, 321, 180)
    batch = _run(m, x)
    head = _run(m, x, fuse_blocks123=0)
    assert torch.equal(batch[0], head[0])
    for i in (0, 137, 255):
        one = _run(m, x[i:i + 1])
        assert torch.equal(one[0][0], batch[0][i]), i
        assert torch.equal(one[1][0], batch[1][i]), i
