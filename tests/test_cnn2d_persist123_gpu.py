"""CNN2D bf16 eval forward: the blocks 1-3 kernel as one persistent workgroup per CU (conv123_persist.hip, context option
"persist123").  It must reproduce the per-unit kernel (conv123_fused.hip, persist123 = 0) bit for bit -- logits and
embeddings -- for every shape the dispatcher fuses, its compiler-scheduled twin must equal the pipelined build, stale LDS
must not matter, and nothing may leak from one unit of a workgroup's range into the next."""
import pytest
import torch

from conv123_common import PATTERNS, _ctx, _model, _probe_workgroups, _restore_options, _run, _same, _slots, _x  # noqa: F401 (_restore_options: autouse)

pytestmark = pytest.mark.gpu


SHAPES = [
    # the eight shapes of test_fused123_bit_identical_to_two_kernel_path
    (256, 321, 180, torch.bfloat16, True),      # the headline: six units = one utterance per workgroup on 256 CUs
    (200, 321, 180, torch.bfloat16, True),      # 1200 units: not a multiple of the grid
    (256, 321, 47, torch.bfloat16, True),       # two strips per utterance, ragged last strip: ranges cross utterances
    (192, 321, 65, torch.bfloat16, True),       # three strips per utterance
    (256, 322, 180, torch.bfloat16, True),      # odd H1 / H2 splits
    (256, 33, 180, torch.bfloat16, True),       # short T (niter3 = 4)
    (256, 321, 180, torch.bfloat16, False),     # contiguous [B, T, F]
    (256, 321, 180, torch.float32, True),       # fp32 features, rounded to bf16 on load
    # ranges of two and three units
    (86, 321, 180, torch.bfloat16, True),       # 516 units
    # niter3 = 40, 41, 41, 42, 43: every residue mod 4 and mod 3; T = 329 has an odd H2
    (256, 325, 180, torch.bfloat16, True),
    (256, 329, 180, torch.bfloat16, True),
    (256, 337, 180, torch.bfloat16, True),
    (256, 345, 180, torch.bfloat16, True),
    (256, 329, 65, torch.bfloat16, True),
    (256, 337, 47, torch.float32, False),
]


@pytest.mark.parametrize("B,T,F,dtype,strided", SHAPES)
def test_persist123_bit_identical_to_per_unit_kernel(B, T, F, dtype, strided):
    m = _model(F)
    x = _x(B, T, F, dtype=dtype, strided=strided)
    want = _run(m, x, persist123=0)
    got = _run(m, x, persist123=1)
    assert torch.isfinite(got[0]).all()
    _same(got, want, (B, T, F))


@pytest.mark.parametrize("B,T,F", [(256, 321, 180), (200, 325, 180), (256, 337, 47)])
def test_persist123_bit_identical_to_two_kernel_path(B, T, F):
    m = _model(F)
    x = _x(B, T, F)
    want = _run(m, x, fuse_blocks123=0)
    got = _run(m, x, fuse_blocks123=1, persist123=1)
    _same(got, want, (B, T, F))


@pytest.mark.parametrize("B,T,F", [(256, 321, 180), (200, 329, 65)])
def test_persist123_compiler_scheduled_twin(B, T, F):
    m = _model(F)
    x = _x(B, T, F)
    want = _run(m, x, persist123=1, lds_pipe=1)
    got = _run(m, x, persist123=1, lds_pipe=0)
    _same(got, want, (B, T, F))
    _same(got, _run(m, x, persist123=0, lds_pipe=0), "per-unit twin")


def test_persist123_ignores_stale_lds():
    m = _model(47)
    x = _x(256, 321, 47)
    want = _run(m, x, persist123=0)
    for pat in PATTERNS:
        _ctx().set_option("poison_lds", pat)
        got = _run(m, x, persist123=1)
        _same(got, want, hex(pat))


@pytest.mark.parametrize("B,T,F", [(256, 321, 180), (200, 321, 180), (256, 325, 47)])
def test_persist123_batch_permutation(B, T, F):
    """A permuted batch puts every utterance into another workgroup's range, beside other neighbours: its outputs move with it."""
    m = _model(F)
    x = _x(B, T, F)
    base = _run(m, x, persist123=1)
    perm = torch.randperm(B, generator=torch.Generator().manual_seed(3)).to("cuda")
    xp = x.transpose(1, 2)[perm].contiguous().transpose(1, 2)           # same [B, F, T] storage layout
    got = _run(m, xp, persist123=1)
    _same(got, (base[0][perm], base[1][perm]), (B, T, F))


@pytest.mark.parametrize("fill", [float("nan"), 3e38])
@pytest.mark.parametrize("B,T,F,victim", [(256, 321, 180, 100), (200, 321, 180, 57), (256, 325, 47, 129)])
def test_persist123_no_leak_between_units(B, T, F, victim, fill):
    """One utterance of NaN (or of 3e38, which overflows inside the network) changes no other utterance's output: nothing of a
    unit -- ring rows, windows, running totals, column sums -- survives into the next unit of the same workgroup."""
    m = _model(F)
    x = _x(B, T, F)
    base = _run(m, x, persist123=1)
    stored = x.transpose(1, 2).clone()
    stored[victim] = fill
    got = _run(m, stored.transpose(1, 2), persist123=1)
    keep = torch.ones(B, dtype=torch.bool, device="cuda")
    keep[victim] = False
    assert torch.equal(got[0][keep], base[0][keep]), (got[0][keep] - base[0][keep]).abs().max().item()
    assert torch.equal(got[1][keep], base[1][keep])
    assert not torch.isfinite(got[1][victim]).all() or not torch.equal(got[1][victim], base[1][victim])


def test_persist123_dispatch():
    """Default options: one fused kernel in timing slot 2 + the classifier, and that kernel is the persistent one (the held-clock
    probe reports one workgroup per CU); persist123 = 0: the per-unit kernel (one workgroup per unit, the first 1024 report)."""
    m = _model(180)
    x = _x(256, 321, 180)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    assert _slots(m, x) == [0, 0, 1, 1]
    assert _probe_workgroups(m, x) == min(256 * 6, cus)
    _ctx().set_option("persist123", 0)
    assert _slots(m, x) == [0, 0, 1, 1]
    assert _probe_workgroups(m, x) == min(256 * 6, 1024)
    _ctx().set_option("persist123", 1)
    assert _slots(m, _x(8, 321, 180)) == [0, 1, 1, 1]          # small batch: the time-split two-kernel path, as before
    _ctx().set_option("fuse_blocks123", 0)
    assert _slots(m, x) == [0, 1, 1, 1]
