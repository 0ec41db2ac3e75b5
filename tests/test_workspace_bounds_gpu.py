"""Workspace bounds of every entry point of the C ABI: each path runs once on a roomy workspace of finite bytes and once on a
workspace of EXACTLY the planner's byte count, NaN-filled, between two canary bands (tests/workspace_bands.py).  Asserted:
  (a) both bands survive: no kernel stores a byte outside the size the ABI states (a tile's dead lanes, a forgotten slab);
  (b) every output of the banded run is bit-identical (torch.equal) to the roomy run's: no kernel reads a workspace slot nobody
      wrote (a halo row, the partial sum of a segment that did not run) -- the roomy workspace holds finite bytes there, the
      banded one NaN.
All these paths are deterministic (no atomics), so nothing here rests on a tolerance.  Training steps start both runs from the same
state: a deep copy of the model, the dropout stream reset.  The last tests pin the planners and the entry points' checks to the
same number: a workspace one byte short of the plan is refused (DFA_E_WORKSPACE) with the bands and the outputs untouched.
Options are those of include/dfa_hip.h; every test restores them."""
import copy
import ctypes as C
import random

import numpy as np
import pytest
import torch

import dlqueen_train_oracle as DQ
import workspace_bands as WB

pytestmark = pytest.mark.gpu


def _ctx():
    from dfa_amd import _lib
    return _lib.Context.get(torch.device("cuda"))


def _same(got, want, what):
    assert len(got) == len(want), what
    differ = [i for i, (g, w) in enumerate(zip(got, want)) if g.shape != w.shape or not torch.equal(g, w)]
    assert not differ, f"{what}: outputs {differ} of {len(got)} differ between the NaN-filled exact-size workspace and the roomy one (a stale workspace read)"


def _eval_twice(ctx, planner, run, what, floor=0):
    """run() on a roomy workspace of finite bytes, then inside banded(planner()); bands intact and outputs bit-identical"""
    nbytes = max(int(planner()), floor)
    assert nbytes > 0, what
    own = ctx._ws                                   # the context's ordinary workspace: back in place when this returns
    try:
        ctx._ws = WB.roomy(nbytes)
        want = [t.clone() for t in run()]
        with WB.eval_workspace(ctx, nbytes) as check:
            got = [t.clone() for t in run()]
            check(what)
    finally:
        ctx._ws = own
    _same(got, want, what)


class _options:
    """`with _options(ctx, name=value, ...)`: the context options set for the duration, their defaults restored after.  The ABI has
    no getter, so the defaults stand here (include/dfa_hip.h) and an option that is not listed is refused, not restored to a guess."""
    DEFAULTS = {"time_split": -1, **dict.fromkeys(
        ("fuse_conv1", "block3_m16", "fuse_blocks123", "persist123", "carry_a1", "cnn1d_fused", "cae_dec_fused", "cae_enc1_mfma", "cae_enc_dma",
         "conv1_mfma", "dgrad_m16", "conv1_bwd_fused", "cnn1d_train_x3", "cae_dgrad_mfma", "cae_conv_stats", "cae_bwd_fold", "cae_enc4_wide"), 1)}

    def __init__(self, ctx, **opts):
        unknown = sorted(set(opts) - set(self.DEFAULTS))
        assert not unknown, f"_options knows no default for {unknown}: add it to DEFAULTS from include/dfa_hip.h"
        self.ctx, self.opts = ctx, opts

    def __enter__(self):
        for k, v in self.opts.items():
            self.ctx.set_option(k, v)

    def __exit__(self, *exc):
        for k in self.opts:
            self.ctx.set_option(k, self.DEFAULTS[k])


def _tag(**kw):
    return " ".join(f"{k}={v}" for k, v in kw.items())


# ================================================================================================================ the bands themselves
def test_the_bands_notice_one_byte_on_either_side_and_the_interior_is_nan():
    n = 1000 * 256 + 768
    view, check = WB.banded(n)
    assert view.numel() == n and view.data_ptr() % 256 == 0
    assert bool(view.view(torch.bfloat16).isnan().all()) and bool(view.view(torch.float32).isnan().all())
    assert bool(torch.isfinite(WB.roomy(n).view(torch.float32)).all()) and bool(torch.isfinite(WB.roomy(n).view(torch.bfloat16)).all())
    check("untouched")
    base, off = view._base, view.storage_offset()
    assert off >= max(WB.MIB, n) and base.numel() - off - n >= max(WB.MIB, n)
    view[-1] = 0                                    # the last byte of the workspace is the caller's to write
    check("interior written")
    base[off + n + 5] = 0x5B
    with pytest.raises(AssertionError, match=r"BEHIND the workspace.*first at end\+5, last at end\+5"):
        check("one byte behind")
    base[off + n + 5] = 0x5A
    base[off - 1] = 0
    base[off - 300] = 0
    with pytest.raises(AssertionError, match=rf"IN FRONT OF the workspace.*first at end-{n + 300}, last at end-{n + 1} "):
        check("two bytes in front")


# ================================================================================================================ CNN2D eval
CNN2D_SHAPES = [(1, 4, 180), (2, 5, 180), (5, 33, 65), (2, 33, 5), (3, 130, 36), (2, 323, 180), (33, 7, 180)]
_models = {}


def _cnn2d(F, precision):
    from dfa_amd.model import CNN2D
    if ("cnn2d", F) not in _models:
        torch.manual_seed(100 + F)
        m = CNN2D(in_features=F)
        g = torch.Generator().manual_seed(F)
        with torch.no_grad():
            for i in (1, 6, 11):
                m.conv[i].running_mean.copy_(0.2 * torch.randn(m.conv[i].running_mean.shape, generator=g))
                m.conv[i].running_var.copy_(0.5 + torch.rand(m.conv[i].running_var.shape, generator=g))
        _models["cnn2d", F] = m.to("cuda").eval()
    return _models["cnn2d", F].set_precision(precision)


def _inputs(B, T, F):
    """fp32 contiguous [B,T,F], and the same values in bf16 as the transposed view of the stored [B,F,T]"""
    g = torch.Generator().manual_seed(B * 100000 + T * 1000 + F)
    stored = torch.randn(B, F, T, generator=g) * 3.2 - 0.07
    return {"f32_btf": stored.transpose(1, 2).contiguous().to("cuda"),
            "bf16_bft_view": stored.to("cuda", torch.bfloat16).transpose(1, 2)}


def _cnn2d_case(ctx, m, x, emb, what, lengths=None, form=None):
    from dfa_amd import _lib
    B, T, F = x.shape
    prec = _lib.PRECISIONS[m.precision]
    planner = ctx.lib.dfa_workspace_bytes if lengths is None else ctx.lib.dfa_ragged_workspace_bytes

    def run():
        out = m(x, return_embedding=emb, lengths=lengths)
        if form is not None:
            assert ctx.last_conv123_form() == form, f"{what}: blocks 1-3 ran form {ctx.last_conv123_form()}, the case is about form {form}"
        return out if emb else (out,)
    _eval_twice(ctx, lambda: planner(ctx.handle, _lib.MODEL_CNN2D, B, T, F, prec), run, what)


@pytest.mark.parametrize("precision", ["fp32", "bf16", "bf16x3"])
@pytest.mark.parametrize("B,T,F", CNN2D_SHAPES)
def test_cnn2d_eval_stays_inside_its_workspace(B, T, F, precision):
    ctx = _ctx()
    m = _cnn2d(F, precision)
    for layout, x in _inputs(B, T, F).items():
        for emb in (False, True):
            _cnn2d_case(ctx, m, x, emb, f"cnn2d eval {precision} [{B},{T},{F}] x={layout} embedding={emb}")


@pytest.mark.parametrize("opts", [{"time_split": 0}, {"time_split": 2}, {"time_split": 4}, {"fuse_conv1": 0}, {"block3_m16": 0}],
                         ids=lambda o: _tag(**o))
@pytest.mark.parametrize("B,T,F", CNN2D_SHAPES)
def test_cnn2d_bf16_eval_options_stay_inside_their_workspace(B, T, F, opts):
    ctx = _ctx()
    m = _cnn2d(F, "bf16")
    with _options(ctx, **opts):
        for layout, x in _inputs(B, T, F).items():
            for emb in (False, True):
                _cnn2d_case(ctx, m, x, emb, f"cnn2d eval bf16 {_tag(**opts)} [{B},{T},{F}] x={layout} embedding={emb}")


# B * strips >= 512 reaches the one-kernel forms of blocks 1-3: 86 * 6 = 516 units run the persistent form (2), 256 * 6 = 1536 =
# 6 per CU the carry / phase form (3); with an option cleared the same batch runs form 0 (two kernels), 1 (one workgroup per unit)
# or 2.  The form is asserted, so a case cannot silently test another kernel.
@pytest.mark.parametrize("B,opts,form", [(86, {}, 2), (86, {"fuse_blocks123": 0}, 0), (86, {"persist123": 0}, 1), (86, {"carry_a1": 0}, 2),
                                         (256, {}, 3), (256, {"fuse_blocks123": 0}, 0), (256, {"persist123": 0}, 1), (256, {"carry_a1": 0}, 2)],
                         ids=lambda v: _tag(**v) or "default" if isinstance(v, dict) else str(v))
def test_cnn2d_bf16_one_kernel_forms_stay_inside_their_workspace(B, opts, form):
    ctx = _ctx()
    m = _cnn2d(180, "bf16")
    x = _inputs(B, 33, 180)["bf16_bft_view"]
    with _options(ctx, **opts):
        for emb in (False, True):
            _cnn2d_case(ctx, m, x, emb, f"cnn2d eval bf16 {_tag(**opts)} [{B},33,180] embedding={emb}", form=form)


@pytest.mark.parametrize("B,T,F,lengths", [(5, 37, 180, [4, 37, 36, 5, 21]), (5, 37, 65, [37, 4, 7, 22, 35]),
                                           (86, 33, 180, [4 + (29 * b) % 30 for b in range(85)] + [33])])
def test_cnn2d_ragged_stays_inside_its_workspace(B, T, F, lengths):
    ctx = _ctx()
    m = _cnn2d(F, "bf16")
    for layout, x in _inputs(B, T, F).items():
        for emb in (False, True):
            _cnn2d_case(ctx, m, x, emb, f"cnn2d ragged [{B},{T},{F}] x={layout} embedding={emb}", lengths=lengths)


# ================================================================================================================ CNN1D eval
def _cnn1d(F):
    from dfa_amd.model_cnn1d import CNN1D
    if ("cnn1d", F) not in _models:
        torch.manual_seed(200 + F)
        m = CNN1D(in_features=F)
        g = torch.Generator().manual_seed(F)
        with torch.no_grad():
            for i in (1, 5, 9):
                m.conv[i].running_mean.copy_(0.2 * torch.randn(m.conv[i].running_mean.shape, generator=g))
                m.conv[i].running_var.copy_(0.5 + torch.rand(m.conv[i].running_var.shape, generator=g))
        _models["cnn1d", F] = m.to("cuda").eval()
    return _models["cnn1d", F]


def _cnn1d_case(ctx, m, x, what, lengths=None):
    from dfa_amd import _lib
    B, T, F = x.shape
    planner = ctx.lib.dfa_workspace_bytes if lengths is None else ctx.lib.dfa_ragged_workspace_bytes
    _eval_twice(ctx, lambda: planner(ctx.handle, _lib.MODEL_CNN1D, B, T, F, _lib.PREC_F32), lambda: (m(x, lengths=lengths),), what)


@pytest.mark.parametrize("fused", [1, 2, 0])        # 0 = the three-launch path: the one that uses the h1 / h2 regions
@pytest.mark.parametrize("B,T,F", [(2, 1, 180), (2, 3, 4), (3, 33, 8), (4, 100, 44), (2, 384, 180), (2, 385, 180)])
def test_cnn1d_eval_stays_inside_its_workspace(B, T, F, fused):
    ctx = _ctx()
    m = _cnn1d(F)
    g = torch.Generator().manual_seed(B * 1000 + T + F)
    stored = torch.randn(B, F, T, generator=g) * 3.2 - 0.07
    layouts = {"bft_view": stored.to("cuda").transpose(1, 2), "btf": stored.transpose(1, 2).contiguous().to("cuda")}
    with _options(ctx, cnn1d_fused=fused):
        for layout, x in layouts.items():
            _cnn1d_case(ctx, m, x, f"cnn1d eval cnn1d_fused={fused} [{B},{T},{F}] x={layout}")


def test_cnn1d_ragged_stays_inside_its_workspace():
    ctx = _ctx()
    F = 180
    window = max(t for t in range(3, 400) if ctx.lib.dfa_cnn1d_ragged_segments(t, F, None, None, None, None, 0) == 1)
    lengths = [3, window, window + 1, 37, 385]      # one window's worth, one frame more (two segments), and above 348
    assert max(lengths) > 348
    T = max(lengths)
    g = torch.Generator().manual_seed(7)
    stored = torch.randn(len(lengths), F, -(-T // 4) * 4, generator=g) * 3.2 - 0.07
    layouts = {"bft_view": stored.to("cuda").transpose(1, 2)[:, :T], "btf": stored.transpose(1, 2)[:, :T].contiguous().to("cuda")}
    for layout, x in layouts.items():
        _cnn1d_case(ctx, _cnn1d(F), x, f"cnn1d ragged {lengths} x={layout}", lengths=lengths)
    _cnn1d_case(ctx, _cnn1d(8), torch.randn(3, 8, 36, generator=g).to("cuda").transpose(1, 2)[:, :33], "cnn1d ragged F=8", lengths=[3, 33, 17])


# ================================================================================================================ CAE eval
CAE_SHAPES = [(1, 16, 20), (3, 17, 36), (2, 31, 20), (5, 70, 180), (2, 322, 180)]
CAE_OPTIONS = [{}, {"cae_dec_fused": 0}, {"cae_enc1_mfma": 0}, {"cae_enc_dma": 0}, {"cae_dec_fused": 0, "cae_enc1_mfma": 0, "cae_enc_dma": 0}]


def _cae(precision):
    from dfa_amd.model_cae import ConvAutoencoder
    if "cae" not in _models:
        torch.manual_seed(300)
        m = ConvAutoencoder()
        g = torch.Generator().manual_seed(3)
        with torch.no_grad():
            for n, b in m.named_buffers():
                if n.endswith("running_mean"):
                    b.copy_(0.2 * torch.randn(b.shape, generator=g))
                elif n.endswith("running_var"):
                    b.copy_(0.5 + torch.rand(b.shape, generator=g))
        _models["cae"] = m.to("cuda").eval()
    return _models["cae"].set_precision(precision)


def _cae_cases(ctx, m, B, T, F, what):
    from dfa_amd import _lib
    prec = _lib.PRECISIONS[m.precision]
    g = torch.Generator().manual_seed(B * 1000 + T + F)
    x = (torch.randn(B, T, F, generator=g)).to("cuda")
    raw = x * 2.5 + 1.0
    mean, std = torch.full((F,), 1.0, device="cuda"), torch.full((F,), 2.5, device="cuda")
    planner = lambda: ctx.lib.dfa_workspace_bytes(ctx.handle, _lib.MODEL_CAE, B, T, F, prec)      # noqa: E731
    _eval_twice(ctx, planner, lambda: m(x), what + " forward", floor=256)
    _eval_twice(ctx, planner, lambda: (m.score(x),), what + " score", floor=256)
    _eval_twice(ctx, planner, lambda: (m.score(raw, mean, std),), what + " score with the fused z-score", floor=256)
    _eval_twice(ctx, planner, lambda: (m.score(raw.to(torch.bfloat16), mean, std),), what + " score of bf16 features with the fused z-score",
                floor=256)


@pytest.mark.parametrize("B,T,F", CAE_SHAPES)
def test_cae_fp32_eval_stays_inside_its_workspace(B, T, F):
    _cae_cases(_ctx(), _cae("fp32"), B, T, F, f"cae eval fp32 [{B},{T},{F}]")


@pytest.mark.parametrize("opts", CAE_OPTIONS, ids=lambda o: _tag(**o) or "default")
@pytest.mark.parametrize("B,T,F", CAE_SHAPES)
def test_cae_bf16_eval_stays_inside_its_workspace(B, T, F, opts):
    ctx = _ctx()
    with _options(ctx, **opts):
        _cae_cases(ctx, _cae("bf16"), B, T, F, f"cae eval bf16 {_tag(**opts)} [{B},{T},{F}]")


@pytest.mark.parametrize("B,T,F,lengths", [(3, 17, 36, [16, 17, 16]), (5, 70, 180, [16, 70, 33, 48, 69]), (2, 322, 180, [16, 322]),
                                           (2, 31, 20, [31, 16])])
def test_cae_ragged_score_stays_inside_its_workspace(B, T, F, lengths):
    from dfa_amd import _lib
    ctx = _ctx()
    m = _cae("bf16")
    g = torch.Generator().manual_seed(B * 1000 + T + F + 1)
    raw = (torch.randn(B, T, F, generator=g) * 2.5 + 1.0).to("cuda")
    mean, std = torch.full((F,), 1.0, device="cuda"), torch.full((F,), 2.5, device="cuda")
    planner = lambda: ctx.lib.dfa_cae_ragged_workspace_bytes(ctx.handle, B, T, F, _lib.PREC_BF16)      # noqa: E731
    what = f"cae ragged score [{B},{T},{F}] lengths {lengths}"
    _eval_twice(ctx, planner, lambda: (m.score(raw, lengths=lengths),), what, floor=256)
    _eval_twice(ctx, planner, lambda: (m.score(raw, mean, std, lengths=lengths),), what + " with the fused z-score", floor=256)
    _eval_twice(ctx, planner, lambda: (m.score(raw.to(torch.bfloat16), mean, std, lengths=lengths),), what + " bf16 features", floor=256)


# ================================================================================================================ DeepfakeDetector eval
def _dlq(C_in):
    from dfa_amd.dlqueen_model import DeepfakeDetector
    if ("dlq", C_in) not in _models:
        m = DeepfakeDetector(C_in)
        m.load_state_dict(DQ.make_state_dict(DeepfakeDetector, C_in))
        _models["dlq", C_in] = m.to("cuda").eval()
    return _models["dlq", C_in]


def _dlq_batch(B, C_in, T, seed):
    g = torch.Generator().manual_seed(seed)
    buf = torch.randn(B, C_in, -(-T // 4) * 4, generator=g) * 3.2 - 0.07
    return buf.to("cuda")[:, :, :T]


# around the frame tile NF = 64 of dlq_api.hip (tests/test_dlqueen_gpu.py: one utterance of NF - 1, NF, NF + 1, 2 NF + 1 frames with
# 0 .. 3 frames of padding), mixed batches, and T_max that is no multiple of NF (65, 100, 130)
DLQ_CASES = [(180, n + pad, [n]) for n in (63, 64, 65, 129) for pad in (0, 1, 2, 3)] + \
            [(180, 65, [65, 64, 1]), (180, 130, [130, 129, 67, 33, 3]), (180, 100, [100, 1, 37]), (8, 5, [5, 2])]


@pytest.mark.parametrize("C_in,T,lengths", DLQ_CASES)
def test_deepfake_detector_eval_stays_inside_its_workspace(C_in, T, lengths):
    from dfa_amd import dlqueen_model as M
    assert M.TILE_FRAMES == 64
    ctx = _ctx()
    m = _dlq(C_in)
    B = len(lengths)
    x = _dlq_batch(B, C_in, T, 50 + T)
    _eval_twice(ctx, lambda: ctx.lib.dfa_dlq_workspace_bytes(ctx.handle, B, T, C_in), lambda: m(x, lengths, return_pooled=True),
                f"DeepfakeDetector eval C={C_in} T_max={T} lengths {lengths}")


# ================================================================================================================ training steps
def _bn_buffers(m):
    return [b for n, b in m.named_buffers() if "running_" in n]


def _train_twice(base, nbytes, step, what):
    """step(model) -> outputs, on a deep copy of `base` with a roomy finite workspace and on another inside banded(nbytes)"""
    assert nbytes > 0, what
    runs = []
    for banded in (False, True):
        m = copy.deepcopy(base).train()
        m._drop_seed, m._drop_offset = 5, 0
        if not banded:
            m._train_ws = WB.roomy(nbytes)
            runs.append([t.clone() for t in step(m)])
        else:
            with WB.train_workspace(m, nbytes) as check:
                runs.append([t.clone() for t in step(m)])
                check(what)
        torch.cuda.synchronize()
    _same(runs[1], runs[0], what)


def _classifier_steps(x, y, dlogits, lengths=None, arm=None):
    """(raw forward_train + backward_raw, one NativeTrainer step) as step functions; `arm` runs before every forward"""
    from dfa_amd.training.train_step import NativeTrainer, backward_raw, forward_train_raw

    def raw(m):
        if arm:
            arm()
        (logits,), st = forward_train_raw(m, x, lengths=lengths)
        grads = [torch.full_like(p, float("nan")) for p in m.parameters()]
        backward_raw(m, x, dlogits, grads, st)
        return [logits, *grads, *_bn_buffers(m)]

    def trainer(m):
        tr = NativeTrainer(m, lr=1e-3, weight_decay=0.01, label_smoothing=0.05)
        if arm:
            arm()
        loss = tr.step(x, y, lengths=lengths)
        return [loss, tr.flat_g, tr.flat_p, *_bn_buffers(m)]
    return raw, trainer


def _labels(B, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.arange(B) % 2).float().to("cuda"), (0.3 * torch.randn(B, 1, generator=g)).to("cuda")


CNN2D_TRAIN = [("fp32", {}), ("bf16", {}), ("bf16", {"conv1_mfma": 0}), ("bf16", {"dgrad_m16": 0}), ("bf16", {"conv1_bwd_fused": 0}),
               ("bf16", "augment_folded")]


@pytest.mark.parametrize("precision,opts", CNN2D_TRAIN, ids=lambda v: v if isinstance(v, str) else (_tag(**v) or "default"))
@pytest.mark.parametrize("B,T,F", [(3, 21, 65), (2, 33, 5), (2, 323, 180)])
def test_cnn2d_training_step_stays_inside_its_workspace(B, T, F, precision, opts):
    from dfa_amd import _lib
    from dfa_amd.augmentation import FusedAugment
    from dfa_amd.model import CNN2D
    ctx = _ctx()
    torch.manual_seed(400 + F)
    base = CNN2D(in_features=F, dropout=0.0, precision=precision).to("cuda")
    g = torch.Generator().manual_seed(T * 1000 + F)
    stored = torch.randn(B, F, T, generator=g) * 3.2 - 0.07
    x = stored.to("cuda", torch.bfloat16 if precision == "bf16" else torch.float32).transpose(1, 2)
    y, dlogits = _labels(B, T)
    arm = None
    if opts == "augment_folded":
        def arm():
            random.seed(41); torch.manual_seed(41)
            FusedAugment(seed=5, fold=True, spec_augment=True, time_mask_ratio=0.2, feature_mask=True, feature_mask_ratio=0.1, time_shift=True,
                         time_shift_ratio=0.1, channel_drop=True, channel_drop_prob=0.3)(x)
        opts = {}
    nbytes = ctx.lib.dfa_cnn2d_train_workspace_bytes(ctx.handle, B, T, F, _lib.PRECISIONS[precision])
    what = f"cnn2d train {precision} {_tag(**opts)}{' folded augmentation' if arm else ''} [{B},{T},{F}]"
    with _options(ctx, **opts):
        for name, step in zip(("raw", "NativeTrainer"), _classifier_steps(x, y, dlogits, arm=arm)):
            _train_twice(base, nbytes, step, f"{what} {name}")


@pytest.mark.parametrize("x3", [1, 0])
@pytest.mark.parametrize("B,T,F,lengths", [(2, 37, 180, None), (3, 33, 8, None), (4, 40, 180, [40, 3, 17, 33]), (3, 33, 8, [3, 33, 4])])
def test_cnn1d_training_step_stays_inside_its_workspace(B, T, F, lengths, x3):
    from dfa_amd.model_cnn1d import CNN1D
    ctx = _ctx()
    torch.manual_seed(500 + F)
    base = CNN1D(in_features=F, dropout=0.0).to("cuda")
    g = torch.Generator().manual_seed(T * 1000 + F)
    x = (torch.randn(B, F, -(-T // 4) * 4, generator=g) * 3.2 - 0.07).to("cuda").transpose(1, 2)[:, :T]
    y, dlogits = _labels(B, T)
    planner = ctx.lib.dfa_cnn1d_train_workspace_bytes if lengths is None else ctx.lib.dfa_cnn1d_train_ragged_workspace_bytes
    nbytes = planner(ctx.handle, B, T, F)
    what = f"cnn1d train cnn1d_train_x3={x3} [{B},{T},{F}] lengths {lengths}"
    with _options(ctx, cnn1d_train_x3=x3):
        for name, step in zip(("raw", "NativeTrainer"), _classifier_steps(x, y, dlogits, lengths=lengths)):
            _train_twice(base, nbytes, step, f"{what} {name}")
        xc = x.contiguous()                           # a contiguous [B,T,F] batch: the strided kernels
        for name, step in zip(("raw", "NativeTrainer"), _classifier_steps(xc, y, dlogits, lengths=lengths)):
            _train_twice(base, nbytes, step, f"{what} contiguous btf {name}")


CAE_TRAIN_OPTIONS = ["cae_dgrad_mfma", "conv1_mfma", "dgrad_m16", "cae_conv_stats", "cae_bwd_fold", "cae_enc4_wide"]
_cae_train_base = {}


@pytest.mark.parametrize("option", [None] + CAE_TRAIN_OPTIONS)
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("B,T,F", [(3, 96, 180), (5, 48, 36), (2, 17, 20)])
def test_cae_training_step_stays_inside_its_workspace(B, T, F, precision, option):
    """Raw forward_train + backward and one CaeNativeTrainer step; [2,17,20] is the smallest batch the step takes (T = 17 drops a
    frame at the first pool, F = 20 is a single 32-column chunk, the decoder's first GEMM has two rows)."""
    from dfa_amd import _lib
    from dfa_amd.model_cae import ConvAutoencoder
    from dfa_amd.training.train_step import CaeNativeTrainer, backward_raw, forward_train_raw
    ctx = _ctx()
    if precision not in _cae_train_base:
        torch.manual_seed(600)
        _cae_train_base[precision] = ConvAutoencoder(precision=precision).to("cuda")
    base = _cae_train_base[precision]
    g = torch.Generator().manual_seed(B * 7 + T)
    x = torch.randn(B, T, F, generator=g).to("cuda", torch.bfloat16 if precision == "bf16" else torch.float32)
    drecon = (torch.randn(B, T, F, generator=g) / (B * T * F)).to("cuda")

    def raw(m):
        outs, st = forward_train_raw(m, x, want=("recon", "latent", "mse"))
        grads = [torch.full_like(p, float("nan")) for p in m.parameters()]
        backward_raw(m, x, drecon, grads, st)
        return [*outs, *grads, *_bn_buffers(m)]

    def trainer(m):
        tr = CaeNativeTrainer(m, lr=1e-4, weight_decay=1e-4)
        loss = tr.step(x)                                # MSELoss(recon, x): its gradient is formed inside the backward
        return [loss, tr.flat_g, tr.flat_p, *_bn_buffers(m)]
    nbytes = ctx.lib.dfa_cae_train_workspace_bytes(ctx.handle, B, T, F, _lib.PRECISIONS[precision])
    opts = {} if option is None else {option: 0}
    with _options(ctx, **opts):
        for name, step in (("raw", raw), ("CaeNativeTrainer", trainer)):
            _train_twice(base, nbytes, step, f"cae train {precision} {_tag(**opts)} [{B},{T},{F}] {name}")


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("B,T,F", [(2, 17, 20), (8, 48, 20), (5, 48, 36), (3, 96, 180)])
def test_cae_backward_leaves_the_forward_state_in_its_workspace_alone(B, T, F, precision):
    """Two backward calls on ONE forward state give bit-identical gradients: no backward scratch lies over a region of the plan that is
    still live (the saved activations, the BatchNorm batch statistics, the packed weights).  The bands cannot see such an
    overlap, it stays inside the workspace.  At [2,17,20] and [8,48,20] the bf16 ConvTranspose2d data gradient's weight fragments
    (up to 256 KiB) are larger than the P * Cin floats of the fp32 product's region they once shared."""
    from dfa_amd import _lib
    from dfa_amd.model_cae import ConvAutoencoder
    from dfa_amd.training.train_step import backward_raw, forward_train_raw
    ctx = _ctx()
    torch.manual_seed(600)
    m = ConvAutoencoder(precision=precision).to("cuda").train()
    g = torch.Generator().manual_seed(B * 7 + T)
    x = torch.randn(B, T, F, generator=g).to("cuda", torch.bfloat16 if precision == "bf16" else torch.float32)
    drecon = (torch.randn(B, T, F, generator=g) / (B * T * F)).to("cuda")
    what = f"cae backward twice {precision} [{B},{T},{F}]"
    with WB.train_workspace(m, ctx.lib.dfa_cae_train_workspace_bytes(ctx.handle, B, T, F, _lib.PRECISIONS[precision])) as check:
        _, st = forward_train_raw(m, x, want=("mse",))
        first = [torch.full_like(p, float("nan")) for p in m.parameters()]
        again = [torch.full_like(p, float("nan")) for p in m.parameters()]
        backward_raw(m, x, drecon, first, st)
        backward_raw(m, x, drecon, again, st)
        check(what)
    names = [n for n, _ in m.named_parameters()]
    differ = [n for n, a, b in zip(names, first, again) if not torch.equal(a, b)]
    assert not differ, f"{what}: the second backward on the same forward state changed the gradient of {differ}"


@pytest.mark.parametrize("name", ["A", "C"])
def test_deepfake_detector_training_step_stays_inside_its_workspace(name):
    from dfa_amd.dlqueen_model import DeepfakeDetector
    from dfa_amd.training import DlqTrainer
    ctx = _ctx()
    B, C_in, T, _ = DQ.CASES[name]
    xc, lengths, y = DQ.make_case(name)
    base = DeepfakeDetector(C_in, dropout=0.3)
    base.load_state_dict(DQ.make_state_dict(DeepfakeDetector, C_in))
    base = base.to("cuda")
    xb = xc._base if xc._base is not None else xc
    x = xb.to("cuda")[:, :, :T]

    def step(m):
        tr = DlqTrainer(m, lr=1e-3, weight_decay=1e-4, pos_weight=DQ.POS_WEIGHT, grad_clip=5.0, ema_decay=0.999)
        out = []
        for _ in range(2):
            out += [tr.step(x, lengths, y).clone(), tr.flat_g.clone()]
        return [*out, tr.flat_p, tr.shadow, *_bn_buffers(m)]
    _train_twice(base, ctx.lib.dfa_dlq_train_workspace_bytes(ctx.handle, B, T, C_in), step, f"DeepfakeDetector train case {name}")


# ================================================================================================================ boundary refusal
def _refused(ctx, nbytes, call, outputs, what):
    """call(workspace pointer, byte count) with a view of exactly the plan but ONE BYTE LESS stated: DFA_E_WORKSPACE, the bands, the
    interior and the outputs untouched; then the same call with the plan's own count succeeds (the two agree on one number)"""
    from dfa_amd import _lib
    assert nbytes > 0, what
    view, check = WB.banded(nbytes)
    for o in outputs:
        o.fill_(7.0)
    code = call(C.c_void_p(view.data_ptr()), nbytes - 1)
    assert code == _lib.E_WORKSPACE, f"{what}: workspace_bytes = planner - 1 gave {ctx.lib.dfa_error_name(code).decode()}: " \
                                     f"{ctx.lib.dfa_last_error(ctx.handle).decode()}"
    check(what + " (refused call)")
    assert bool((view == 0xFF).all()), f"{what}: a refused call wrote into the workspace"
    for o in outputs:
        assert bool((o == 7.0).all()), f"{what}: a refused call wrote an output"
    _lib.check(ctx.handle, call(C.c_void_p(view.data_ptr()), nbytes))
    check(what + " (accepted call)")


def test_eval_entry_points_refuse_a_workspace_one_byte_short():
    from dfa_amd import _lib
    ctx = _ctx()
    lib, h, P = ctx.lib, ctx.handle, _lib.ptr
    ctx.use_current_stream()
    # CNN2D uniform and ragged (bf16)
    B, T, F = 2, 33, 180
    m = _cnn2d(F, "bf16")
    x = _inputs(B, T, F)["bf16_bft_view"]
    m._ensure_prepared(ctx)
    logits, emb = torch.empty(B, 1, device="cuda"), torch.empty(B, 128 * F, device="cuda")
    head = (h, P(x), _lib.DTYPE_BF16, B, T, F, *x.stride())
    _refused(ctx, lib.dfa_workspace_bytes(h, _lib.MODEL_CNN2D, B, T, F, _lib.PREC_BF16),
             lambda ws, n: lib.dfa_cnn2d_forward(*head, P(logits), P(emb), ws, n), [logits, emb], "dfa_cnn2d_forward")
    ln = np.asarray([4, 33], dtype=np.int32)
    _refused(ctx, lib.dfa_ragged_workspace_bytes(h, _lib.MODEL_CNN2D, B, T, F, _lib.PREC_BF16),
             lambda ws, n: lib.dfa_cnn2d_forward_ragged(*head, C.c_void_p(ln.ctypes.data), P(logits), P(emb), ws, n), [logits, emb],
             "dfa_cnn2d_forward_ragged")
    # CNN1D uniform and ragged (the stored layout)
    B, T, F = 3, 36, 8
    m1 = _cnn1d(F)
    g = torch.Generator().manual_seed(9)
    x1 = torch.randn(B, F, T, generator=g).to("cuda").transpose(1, 2)
    m1._ensure_prepared(ctx)
    logits1 = torch.empty(B, 1, device="cuda")
    head = (h, P(x1), _lib.DTYPE_F32, B, T, F, *x1.stride())
    _refused(ctx, lib.dfa_workspace_bytes(h, _lib.MODEL_CNN1D, B, T, F, _lib.PREC_F32),
             lambda ws, n: lib.dfa_cnn1d_forward(*head, P(logits1), ws, n), [logits1], "dfa_cnn1d_forward")
    ln1 = np.asarray([3, 36, 17], dtype=np.int32)
    _refused(ctx, lib.dfa_ragged_workspace_bytes(h, _lib.MODEL_CNN1D, B, T, F, _lib.PREC_F32),
             lambda ws, n: lib.dfa_cnn1d_forward_ragged(*head, C.c_void_p(ln1.ctypes.data), P(logits1), ws, n), [logits1],
             "dfa_cnn1d_forward_ragged")
    # auto-encoder: forward (reconstruction + latent), score (the per-sample error alone), ragged score
    B, T, F = 3, 17, 36
    ma = _cae("bf16")
    xa = torch.randn(B, T, F, generator=g).to("cuda")
    ma._ensure_prepared(ctx)
    recon, latent, mse = torch.empty(B, T, F, device="cuda"), torch.empty(B, 256, T // 16, F // 16, device="cuda"), torch.empty(B, device="cuda")
    head = (h, P(xa), _lib.DTYPE_F32, B, T, F, *xa.stride())
    need = lib.dfa_workspace_bytes(h, _lib.MODEL_CAE, B, T, F, _lib.PREC_BF16)
    _refused(ctx, need, lambda ws, n: lib.dfa_cae_forward(*head, None, None, P(recon), P(latent), None, ws, n), [recon, latent],
             "dfa_cae_forward")
    _refused(ctx, need, lambda ws, n: lib.dfa_cae_forward(*head, None, None, None, None, P(mse), ws, n), [mse], "dfa_cae_forward (score)")
    lna = np.asarray([16, 17, 16], dtype=np.int32)
    _refused(ctx, lib.dfa_cae_ragged_workspace_bytes(h, B, T, F, _lib.PREC_BF16),
             lambda ws, n: lib.dfa_cae_score_ragged(*head, C.c_void_p(lna.ctypes.data), None, None, P(mse), ws, n), [mse], "dfa_cae_score_ragged")
    # DeepfakeDetector
    C_in, T, lengths = 180, 65, [65, 64, 1]
    md = _dlq(C_in)
    xd = _dlq_batch(3, C_in, T, 3)
    md._ensure_prepared(ctx)
    lg, pooled = torch.empty(3, device="cuda"), torch.empty(3, 512, device="cuda")
    lnd = np.asarray(lengths, dtype=np.int32)
    sb, sc, _ = xd.stride()
    _refused(ctx, lib.dfa_dlq_workspace_bytes(h, 3, T, C_in),
             lambda ws, n: lib.dfa_dlq_forward(h, P(xd), 3, T, C_in, sb, sc, C.c_void_p(lnd.ctypes.data), P(lg), P(pooled), ws, n), [lg, pooled],
             "dfa_dlq_forward")


def test_training_backward_refuses_a_workspace_one_byte_short():
    from dfa_amd.model import CNN2D
    from dfa_amd.model_cae import ConvAutoencoder
    from dfa_amd.model_cnn1d import CNN1D
    from dfa_amd.training.train_step import backward_raw, forward_train_raw
    g = torch.Generator().manual_seed(11)
    cases = [("cnn2d", CNN2D(in_features=5, dropout=0.0), torch.randn(2, 33, 5, generator=g), None),
             ("cnn1d", CNN1D(in_features=8, dropout=0.0), torch.randn(3, 8, 36, generator=g).transpose(1, 2)[:, :33], None),
             ("cnn1d ragged", CNN1D(in_features=8, dropout=0.0), torch.randn(3, 8, 36, generator=g).transpose(1, 2)[:, :33], [3, 33, 4]),
             ("cae", ConvAutoencoder(), torch.randn(2, 17, 20, generator=g), None)]
    for what, m, x, lengths in cases:
        m, x = m.to("cuda").train(), x.to("cuda")
        outs, st = forward_train_raw(m, x, lengths=lengths)
        grads = [torch.full_like(p, 7.0) for p in m.parameters()]
        dout = torch.ones_like(outs[0])
        with pytest.raises(RuntimeError, match="workspace"):
            backward_raw(m, x, dout, grads, st._replace(ws=st.ws[:-1]))
        torch.cuda.synchronize()
        assert all(bool((gr == 7.0).all()) for gr in grads), f"{what}: a refused backward wrote a gradient"
        backward_raw(m, x, dout, grads, st)             # the forward is still in flight: the full workspace is accepted
        torch.cuda.synchronize()
        assert all(bool(torch.isfinite(gr).all()) for gr in grads), what
