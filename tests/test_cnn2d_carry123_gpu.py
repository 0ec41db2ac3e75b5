"""CNN2D bf16 eval forward: the persistent blocks 1-3 kernel with two a1 columns carried from strip to strip
(conv123_carry.hip, context option "carry_a1").  It must reproduce the persistent kernel without the carry, the per-unit
kernel and the two-kernel path bit for bit -- logits and embeddings --, its compiler-scheduled twin must equal the pipelined
build, stale LDS (the side buffer above all) must not matter, nothing may leak from one utterance of a workgroup's range into
the next, and the dispatcher must choose it exactly where every range is a whole number of utterances and the side buffer
fits LDS."""
import pytest
import torch

from conv123_common import CARRY, NONE, PATTERNS, PER_UNIT, PERSIST, _ctx, _cus, _model, _niter3, _restore_options, _run, _same, _x  # noqa: F401 (_restore_options: autouse)

pytestmark = pytest.mark.gpu

# conv123_body.h, namespace c123: the kernel's LDS without the side buffer, and the side buffer's bytes per a1 ring block
CRING_BYTES = 4 * 2 * 32 * 128
P_OFF = CRING_BYTES + 128 * 4 + 256 * 64
P_BYTES = 3 * 4 * 36 * 64 + 64 * 4 + 2 * 10 * 36 * 8 + 16
LDS_BYTES = P_OFF + P_BYTES
SIDE_BLKB = 4 * 2 * 64
LDS_CAP = 160 * 1024


def _fits(T):
    return LDS_BYTES + (_niter3(T) + 2) * SIDE_BLKB <= LDS_CAP


def _identity(B, T, F, **xkw):
    m = _model(F)
    x = _x(B, T, F, **xkw)
    got = _run(m, x, form=CARRY)
    assert torch.isfinite(got[0]).all()
    _same(got, _run(m, x, form=PERSIST, carry_a1=0), (B, T, F, "carry_a1=0"))
    _same(got, _run(m, x, form=PER_UNIT, persist123=0), (B, T, F, "persist123=0"))
    _same(got, _run(m, x, form=NONE, fuse_blocks123=0), (B, T, F, "fuse_blocks123=0"))


SHAPES = [
    (33, 47),      # two strips, ragged last strip
    (41, 61),      # three strips, the last one column wide
    (43, 62),      # three strips
    (45, 90),      # three exact strips
    (40, 180),     # six strips
    (322, 65),     # three strips, odd H1 / H2 splits
]


@pytest.mark.parametrize("per_wg", [1, 2])     # 2: two utterances per workgroup, strip 0 comes after a last strip
@pytest.mark.parametrize("T,F", SHAPES)
def test_carry123_bit_identical(T, F, per_wg):
    _identity(per_wg * _cus(), T, F)


def test_carry123_fp32_features():
    _identity(_cus(), 41, 61, dtype=torch.float32)


def test_carry123_contiguous_features():
    _identity(2 * _cus(), 43, 62, strided=False)


def test_carry123_compiler_scheduled_twin():
    B, T, F = 2 * _cus(), 41, 61
    m = _model(F)
    x = _x(B, T, F)
    want = _run(m, x, form=CARRY, lds_pipe=1)
    got = _run(m, x, form=CARRY, lds_pipe=0)
    _same(got, want, (B, T, F))
    _same(got, _run(m, x, form=PERSIST, carry_a1=0, lds_pipe=0), "persistent twin")


def test_carry123_ignores_stale_lds():
    B, T, F = _cus(), 33, 47
    m = _model(F)
    x = _x(B, T, F)
    want = _run(m, x, form=PER_UNIT, persist123=0)
    for pat in PATTERNS:
        _ctx().set_option("poison_lds", pat)
        _same(_run(m, x, form=CARRY), want, hex(pat))


@pytest.mark.parametrize("fill", [float("nan"), 3e38])
@pytest.mark.parametrize("place", [0, 1])      # the victim is the first / the second utterance of its workgroup's range
def test_carry123_no_leak_between_utterances(place, fill):
    """One utterance of NaN (or of 3e38, which overflows inside the network) changes no other utterance's output: the side
    buffer its last strip leaves behind is not what the next utterance's first strip puts into its ring."""
    cus = _cus()
    B, T, F = 2 * cus, 33, 61
    victim = 2 * (cus // 3) + place            # ranges are utterance pairs (2 w, 2 w + 1)
    m = _model(F)
    x = _x(B, T, F)
    base = _run(m, x, form=CARRY)
    stored = x.transpose(1, 2).clone()
    stored[victim] = fill
    got = _run(m, stored.transpose(1, 2), form=CARRY)
    keep = torch.ones(B, dtype=torch.bool, device="cuda")
    keep[victim] = False
    assert torch.equal(got[0][keep], base[0][keep]), (got[0][keep] - base[0][keep]).abs().max().item()
    assert torch.equal(got[1][keep], base[1][keep])
    assert not torch.isfinite(got[1][victim]).all() or not torch.equal(got[1][victim], base[1][victim])


def test_carry123_dispatch():
    cus = _cus()
    m61, m180, m47 = _model(61), _model(180), _model(47)
    _run(m61, _x(cus, 33, 61), form=CARRY)
    _run(m61, _x(cus, 33, 61), form=PERSIST, carry_a1=0)
    _run(m180, _x(cus - 56, 33, 180), form=PERSIST)                  # units not a multiple of the grid
    assert ((cus + 1) * 3) % cus != 0
    _run(m61, _x(cus + 1, 33, 61), form=PERSIST)
    if cus % 2 == 0:                                                 # three units per workgroup, two strips per utterance
        _run(m47, _x(3 * cus // 2, 33, 47), form=PERSIST)
    _run(m61, _x(cus, 33, 61), form=PER_UNIT, persist123=0)
    _run(m61, _x(cus, 33, 61), form=NONE, fuse_blocks123=0)


def test_carry123_lds_cap():
    """The longest T whose side buffer fits the CU's LDS runs the carry form, the next niter3 the persistent kernel; both
    equal the per-unit kernel."""
    cus = _cus()
    T = 4
    while _fits(T + 1):
        T += 1
    assert _fits(T) and not _fits(T + 1) and _niter3(T + 1) == _niter3(T) + 1
    m = _model(61)
    for t, form in ((T, CARRY), (T + 1, PERSIST)):
        x = _x(cus, t, 61)
        _same(_run(m, x, form=form), _run(m, x, form=PER_UNIT, persist123=0), (t, form))
