"""CNN2D bf16 eval forward: the phase form with the classifier head inside the kernel (conv123_cls.hip, context option
"cls123"; the same cases passed with its build option DFA_C123_LATE_EMIT, the time-mean stores moved off the producers'
step 0, before that part was measured and left out).  It runs linear1_kernel's operation sequence at the end of each workgroup, so logits and embeddings must be the bits of the option at 0 (phase kernel +
linear1_kernel), of phase123 = 0 and of carry_a1 = 0: for one and two utterances per workgroup, T = 4 .. 64 (niter3 = 1, 2, 3, 5,
8: one step, fewer steps than the ring's skew, chunk flushes), F = 30 .. 180 (one strip to six), bf16 and fp32 features, strided
and contiguous, the embedding in the caller's buffer or not asked for.  The dispatcher takes it exactly where the phase form
runs and the classifier's 16-byte path applies, reports it, and launches no classifier behind it."""
import ctypes as C

import pytest
import torch

import workspace_bands as WB
from conv123_common import CARRY, NONE, PER_UNIT, PERSIST, _ctx, _cus, _model, _niter3, _restore_options, _run, _same, _x  # noqa: F401 (_restore_options: autouse)

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _restore_cls123():
    yield
    _ctx().set_option("cls123", 1)


def _run_cls(m, x, cls, want_cls=None, **kw):
    """_run with option cls123 = cls; want_cls: what dfa_ctx_last_conv123_cls must answer (default: cls)"""
    ctx = _ctx()
    ctx.set_option("cls123", cls)
    out = _run(m, x, **kw)
    assert ctx.last_conv123_cls() == (cls if want_cls is None else want_cls), (ctx.last_conv123_cls(), cls, want_cls, kw)
    return out


def _fused(B, F):
    """the dispatcher fuses blocks 1-3 where B * strips >= 512 (cnn2d_api.hip); below that the two-kernel path runs"""
    return B * ((F + 29) // 30) >= 512


def _identity(B, T, F, **xkw):
    m = _model(F)
    x = _x(B, T, F, **xkw)
    if not _fused(B, F):              # (F = 30 at B = CU count on a 256-CU chip: another path, the option selects nothing)
        got = _run_cls(m, x, 1, want_cls=0, form=NONE, phase=0)
        _same(got, _run_cls(m, x, 0, form=NONE, phase=0), (B, T, F, "cls123=0"))
        return
    got = _run_cls(m, x, 1, form=CARRY, phase=1)
    assert torch.isfinite(got[0]).all()
    _same(got, _run_cls(m, x, 0, form=CARRY, phase=1), (B, T, F, "cls123=0"))
    _same(got, _run_cls(m, x, 1, want_cls=0, form=CARRY, phase=0, phase123=0), (B, T, F, "phase123=0"))
    _same(got, _run_cls(m, x, 1, want_cls=0, form=PERSIST, phase=0, carry_a1=0), (B, T, F, "carry_a1=0"))


TS = [(4, 1), (13, 2), (21, 3), (37, 5), (64, 8)]
FS = [30, 31, 61, 180]


@pytest.mark.parametrize("per_wg", [1, 2])
@pytest.mark.parametrize("F", FS)
@pytest.mark.parametrize("T,n", TS)
def test_cls123_bit_identical(T, n, F, per_wg):
    assert _niter3(T) == n
    _identity(per_wg * _cus(), T, F)


@pytest.mark.parametrize("per_wg", [1, 2])
def test_cls123_fp32_features(per_wg):
    _identity(per_wg * _cus(), 21, 61, dtype=torch.float32)


@pytest.mark.parametrize("per_wg", [1, 2])
def test_cls123_contiguous_features(per_wg):
    _identity(per_wg * _cus(), 37, 31, strided=False)


def test_cls123_compiler_scheduled_twin():
    B, T, F = 2 * _cus(), 37, 61
    m = _model(F)
    x = _x(B, T, F)
    want = _run_cls(m, x, 1, form=CARRY, phase=1, lds_pipe=1)
    got = _run_cls(m, x, 1, form=CARRY, phase=1, lds_pipe=0)
    _same(got, want, (B, T, F))
    _same(got, _run_cls(m, x, 0, form=CARRY, phase=1, lds_pipe=0), "phase twin")


# ------------------------------------------------------------------------------------------------------ the raw ABI call
def _raw(m, x, logits, emb, expect_ok=True):
    """dfa_cnn2d_forward with the caller's own logits / embedding buffers (emb None: not requested) -> the ABI's return code"""
    from dfa_amd import _lib
    B, T, F = x.shape
    with _lib.launch(m, x) as ctx:
        lib = ctx.lib
        ws = ctx.workspace(lib.dfa_workspace_bytes(ctx.handle, _lib.MODEL_CNN2D, B, T, F, _lib.PRECISIONS["bf16"]))
        code = lib.dfa_cnn2d_forward(ctx.handle, _lib.ptr(x), _lib.x_dtype_code(x), B, T, F, *x.stride(),
                                     C.c_void_p(logits.data_ptr()), C.c_void_p(emb.data_ptr()) if emb is not None else None,
                                     _lib.ptr(ws), ws.numel())
    torch.cuda.synchronize()
    if expect_ok:
        _lib.check(ctx.handle, code)
    return code


@pytest.mark.parametrize("per_wg", [1, 2])
def test_cls123_overwrites_every_logit_and_needs_no_embedding_request(per_wg):
    """The logits buffer pre-filled with NaN: every entry is written, with and without the embedding requested (without: the
    kernel reads the rows back from the workspace slab)."""
    B, T, F = per_wg * _cus(), 21, 61
    m = _model(F)
    x = _x(B, T, F)
    ctx = _ctx()
    ctx.set_option("cls123", 0)
    want_lg, want_emb = m(x, return_embedding=True)
    ctx.set_option("cls123", 1)
    for with_emb in (True, False):
        lg = torch.full((B, 1), float("nan"), device="cuda")
        emb = torch.full((B, 128 * F), float("nan"), device="cuda") if with_emb else None
        _raw(m, x, lg, emb)
        assert ctx.last_conv123_cls() == 1
        assert torch.equal(lg, want_lg), with_emb
        if with_emb:
            assert torch.equal(emb, want_emb)


@pytest.mark.parametrize("fill", [float("nan"), 3e38])
@pytest.mark.parametrize("place", [0, 1])      # the victim is the first / the second utterance of its workgroup's range
def test_cls123_no_leak_between_utterances(place, fill):
    cus = _cus()
    B, T, F = 2 * cus, 21, 61
    victim = 2 * (cus // 3) + place            # ranges are utterance pairs (2 w, 2 w + 1)
    m = _model(F)
    x = _x(B, T, F)
    base = _run_cls(m, x, 1, form=CARRY, phase=1)
    stored = x.transpose(1, 2).clone()
    stored[victim] = fill
    got = _run_cls(m, stored.transpose(1, 2), 1, form=CARRY, phase=1)
    keep = torch.ones(B, dtype=torch.bool, device="cuda")
    keep[victim] = False
    assert torch.equal(got[0][keep], base[0][keep]), (got[0][keep] - base[0][keep]).abs().max().item()
    assert torch.equal(got[1][keep], base[1][keep])
    assert not torch.isfinite(got[1][victim]).all() or not torch.equal(got[1][victim], base[1][victim])


def _slot3(m, x):
    """(ms, records) of timing slot 3 (emb_reduce + classifier) over one forward, and the record counts of slots 0 .. 3"""
    ctx = _ctx()
    ctx.timing_reset()
    ctx.timing(True)
    m(x)
    torch.cuda.synchronize()
    ctx.timing(False)
    return ctx.timing_read(3), [ctx.timing_read(s)[1] for s in range(4)]


def test_cls123_dispatch():
    cus = _cus()
    m61, m180 = _model(61), _model(180)
    x = _x(cus, 21, 61)
    _run_cls(m61, x, 1, form=CARRY, phase=1)                                        # defaults: in the kernel
    # ... and slot 3 records no launch: the existing dispatch tests pin one record per forward in that slot, so the record stays
    # and stands for an empty stage -- exactly 0 ms, where a launch of linear1_kernel gives a positive time
    assert _slot3(m61, x) == ((0.0, 1), [0, 0, 1, 1])
    _run_cls(m61, x, 0, form=CARRY, phase=1)                                        # option off
    (ms, n), counts = _slot3(m61, x)
    assert ms > 0.0 and n == 1 and counts == [0, 0, 1, 1]
    _run_cls(m61, x, 1, want_cls=0, form=CARRY, phase=0, phase123=0)                # another form runs: the carry kernel,
    _run_cls(m61, x, 1, want_cls=0, form=PERSIST, phase=0, carry_a1=0)              # ... the persistent one,
    _run_cls(m180, _x(cus - 56, 21, 180), 1, want_cls=0, form=PERSIST, phase=0)     # ... units not a multiple of the grid,
    assert ((cus + 1) * 3) % cus != 0
    _run_cls(m61, _x(cus + 1, 21, 61), 1, want_cls=0, form=PERSIST, phase=0)
    _run_cls(m61, x, 1, want_cls=0, form=PER_UNIT, phase=0, persist123=0)           # ... one workgroup per unit,
    _run_cls(m61, x, 1, want_cls=0, form=NONE, phase=0, fuse_blocks123=0)           # ... the two-kernel path


def test_cls123_reporter_after_a_refused_embedding():
    """A misaligned embedding pointer is refused by the forward's buffer check: nothing runs, the reporter reads 0."""
    B, T, F = _cus(), 21, 61
    m = _model(F)
    x = _x(B, T, F)
    ctx = _ctx()
    _run_cls(m, x, 1, form=CARRY, phase=1)
    assert ctx.last_conv123_cls() == 1
    lg = torch.empty((B, 1), device="cuda")
    buf = torch.empty(B * 128 * F + 4, device="cuda")
    code = _raw(m, x, lg, buf[1:], expect_ok=False)                                 # 4 bytes off a 16-byte boundary
    assert code != 0
    assert ctx.last_conv123_cls() == 0


@pytest.mark.parametrize("B_of,T,F", [(lambda c: c, 13, 61), (lambda c: 2 * c, 21, 31)])
def test_cls123_exact_size_workspace(B_of, T, F):
    """tests/workspace_bands.py on the new path: the kernel reads the embedding rows back from the workspace (embedding not
    requested) or from the caller's buffer; bands intact, outputs identical to a roomy workspace of finite bytes."""
    from dfa_amd import _lib
    B = B_of(_cus())
    m = _model(F)
    x = _x(B, T, F)
    ctx = _ctx()
    ctx.set_option("cls123", 1)
    nbytes = int(ctx.lib.dfa_workspace_bytes(ctx.handle, _lib.MODEL_CNN2D, B, T, F, _lib.PRECISIONS["bf16"]))
    own = ctx._ws
    try:
        for with_emb in (False, True):
            run = (lambda: list(m(x, return_embedding=True))) if with_emb else (lambda: [m(x)])
            ctx._ws = WB.roomy(nbytes)
            want = [t.clone() for t in run()]
            assert ctx.last_conv123_cls() == 1
            with WB.eval_workspace(ctx, nbytes) as check:
                got = [t.clone() for t in run()]
                check((B, T, F, with_emb))
            assert ctx.last_conv123_cls() == 1
            assert all(torch.equal(g, w) for g, w in zip(got, want)), (B, T, F, with_emb)
    finally:
        ctx._ws = own
