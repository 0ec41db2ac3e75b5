"""CNN2D bf16 eval forward: the de-phased build of the carry form (conv123_phase.hip, context option "phase123": the
consumers' step barrier behind fragment read 35 instead of read 4, consumer waves at raised issue priority).  It moves a
barrier and computes nothing differently, so logits and embeddings must be bit-identical to the carry form as it was
(phase123 = 0) and to the persistent kernel without the carry (carry_a1 = 0): for one and two utterances per workgroup, for
every niter3 = 1 .. 5 (the a2 ring has four blocks: short units wrap it least and reach the unit boundary soonest), with
stale LDS, and with a NaN utterance next to a clean one.  The dispatcher takes it exactly where it took the carry form and
keeps reporting that form."""
import pytest
import torch

from conv123_common import CARRY, NONE, PATTERNS, PER_UNIT, PERSIST, _ctx, _cus, _model, _niter3, _restore_options, _run, _same, _x  # noqa: F401 (_restore_options: autouse)

pytestmark = pytest.mark.gpu


def _identity(B, T, F, **xkw):
    m = _model(F)
    x = _x(B, T, F, **xkw)
    got = _run(m, x, form=CARRY, phase=1)
    assert torch.isfinite(got[0]).all()
    _same(got, _run(m, x, form=CARRY, phase=0, phase123=0), (B, T, F, "phase123=0"))
    _same(got, _run(m, x, form=PERSIST, phase=0, carry_a1=0), (B, T, F, "carry_a1=0"))


SHAPES = [
    (33, 47),      # two strips, ragged last strip
    (41, 61),      # three strips, the last one column wide
    (43, 62),      # three strips
    (45, 90),      # three exact strips
    (40, 180),     # six strips
    (322, 65),     # three strips, odd H1 / H2 splits
]
# T for niter3 = 2, 3, 5 (H2 = 3, 5, 9: odd, so the last iteration has one live row and the producers' masked row H2), and
# T = 4, the shortest the API accepts (two (2,1) pools) and the carry form with it: H1 = 2, H2 = 1, niter3 = 1, where a unit
# is its two idle steps, one working step and the boundary
SHORT = [(13, 2), (21, 3), (37, 5), (4, 1)]


@pytest.mark.parametrize("per_wg", [1, 2])     # 2: two utterances per workgroup, strip 0 comes after a last strip
@pytest.mark.parametrize("T,F", SHAPES)
def test_phase123_bit_identical(T, F, per_wg):
    _identity(per_wg * _cus(), T, F)


@pytest.mark.parametrize("per_wg", [1, 2])
@pytest.mark.parametrize("T,n", SHORT)
def test_phase123_bit_identical_short_units(T, n, per_wg):
    assert _niter3(T) == n
    _identity(per_wg * _cus(), T, 61)


def test_phase123_fp32_features():
    _identity(_cus(), 41, 61, dtype=torch.float32)


def test_phase123_contiguous_features():
    _identity(2 * _cus(), 43, 62, strided=False)


def test_phase123_compiler_scheduled_twin():
    B, T, F = 2 * _cus(), 41, 61
    m = _model(F)
    x = _x(B, T, F)
    want = _run(m, x, form=CARRY, phase=1, lds_pipe=1)
    got = _run(m, x, form=CARRY, phase=1, lds_pipe=0)
    _same(got, want, (B, T, F))
    _same(got, _run(m, x, form=CARRY, phase=0, phase123=0, lds_pipe=0), "carry twin")


def test_phase123_ignores_stale_lds():
    B, T, F = _cus(), 33, 47
    m = _model(F)
    x = _x(B, T, F)
    want = _run(m, x, form=CARRY, phase=0, phase123=0)
    for pat in PATTERNS:
        _ctx().set_option("poison_lds", pat)
        _same(_run(m, x, form=CARRY, phase=1), want, hex(pat))


@pytest.mark.parametrize("fill", [float("nan"), 3e38])
@pytest.mark.parametrize("place", [0, 1])      # the victim is the first / the second utterance of its workgroup's range
def test_phase123_no_leak_between_utterances(place, fill):
    """One utterance of NaN (or of 3e38, which overflows inside the network) changes no other utterance's output: the
    consumers, now closer behind the producers, still read no a2 row of another unit."""
    cus = _cus()
    B, T, F = 2 * cus, 33, 61
    victim = 2 * (cus // 3) + place            # ranges are utterance pairs (2 w, 2 w + 1)
    m = _model(F)
    x = _x(B, T, F)
    base = _run(m, x, form=CARRY, phase=1)
    stored = x.transpose(1, 2).clone()
    stored[victim] = fill
    got = _run(m, stored.transpose(1, 2), form=CARRY, phase=1)
    keep = torch.ones(B, dtype=torch.bool, device="cuda")
    keep[victim] = False
    assert torch.equal(got[0][keep], base[0][keep]), (got[0][keep] - base[0][keep]).abs().max().item()
    assert torch.equal(got[1][keep], base[1][keep])
    assert not torch.isfinite(got[1][victim]).all() or not torch.equal(got[1][victim], base[1][victim])


def test_phase123_dispatch():
    cus = _cus()
    m61, m180 = _model(61), _model(180)
    _run(m61, _x(cus, 33, 61), form=CARRY, phase=1)                              # default options: the form value is unchanged
    _run(m61, _x(cus, 33, 61), form=CARRY, phase=0, phase123=0)                  # option off: the carry kernel
    _run(m61, _x(cus, 33, 61), form=PERSIST, phase=0, carry_a1=0)                # no carry: the option selects nothing
    _run(m180, _x(cus - 56, 33, 180), form=PERSIST, phase=0)                     # units not a multiple of the grid
    assert ((cus + 1) * 3) % cus != 0
    _run(m61, _x(cus + 1, 33, 61), form=PERSIST, phase=0)
    _run(m61, _x(cus, 33, 61), form=PER_UNIT, phase=0, persist123=0)
    _run(m61, _x(cus, 33, 61), form=NONE, phase=0, fuse_blocks123=0)
