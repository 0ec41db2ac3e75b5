"""The CNN2D training step, kernel stage by kernel stage, on the tensors the GPU itself stored.

One dfa_cnn2d_forward_train + dfa_bce_smooth_fwd_bwd + dfa_cnn2d_backward per case through the C ABI, on a workspace of the test's
own that is exactly the plan's size between canary bands and NaN in every byte beforehand (tests/workspace_bands.py, handed to the
model as model._train_ws); the gradient tensors are NaN beforehand too.  dfa_cnn2d_train_plan says where every stored tensor lies
-- no offset or dimension is restated here -- and after the step the workspace still holds a1, z2, a2, z3, emb, demb, msum, dz3,
da2, dz2, da1, the statistics block and the sums block.  Every stage of tests/cnn2d_stage_oracle.py is then evaluated in float64 on
THOSE operands and compared with what the GPU stored for it, so no error propagates from one kernel into the check of the next
and the conditioning of the network (which holds a whole-step comparison in bf16 mode to 2-4 % of scale) does not enter.

Criteria: the project's own, tests/cae_stage_oracle.py::compare (tests/test_cnn2d_train_stages_cpu.py shows the CPU's float32
stages meet each with an eighth of its cap):
  tensors stored in bf16   every element |got - want| <= 2^-8 |want| + K 2^-24 A; at most 1e-3 of a case's elements not bit-equal
                           to bf16(want); an element whose float64 BatchNorm output lies within the fp32 rounding of its own terms
                           of zero may take either ReLU branch, at most 1e-4 of a tensor may be such.
  fp32 outputs, and every  max |got - want| / scale and relative L2 against float64 within max(1e-5, 8 floor), floor = the CPU's
  stored tensor of the     float32 evaluation of the same stage on the same operands.  Open ReLU decisions enter a sum's bound with
  fp32-precision runs      their own magnitude.  conv.0.bias, conv.5.bias and conv.10.bias (sums that cancel to rounding residue)
                           are measured against the largest channel sum of |dz|.
  integer / bit-exact      msum's counts equal the float64 mask counts except at open decisions (scale 1: a deviation of one
                           count fails); the (S1, S2) records left in `sums` equal the returned dbeta / dgamma bit for bit;
                           num_batches_tracked is incremented.
  the workspace            every region that holds a stored tensor is finite and is read by a stage (the set of names is
                           asserted); the bands are intact.

What a path leaves in the NaN-filled workspace is asserted in EVERY run: `raw` is written exactly when the two-launch 64 <- 128
data gradient runs (dgrad_m16 = 0, or fp32 precision); XX | Xs and the 11-wide block-1 record exactly on the one-pass block-1
backward (conv1_bwd_fused = 1), whose S2 column is 0 exactly on the matrix-core pass (train_conv1_mfma.hip derives it); the
layer-1 (S1, S2) record exactly on the two-pass backward; with dropout the stored da1 is 0 at every dropped position exactly when
the matrix-core block 1 ran (the data-gradient kernel then applies layer 1's keep mask, csrc/train_api.hip `a.drop = dc`).
train_conv_variant (0, 1: csrc/train_api.hip `fwd3_m16 = ... train_conv_variant() != 1` selects the 16x16x32 30-column-strip
kernel or the 32x32x16 32-column one; csrc/train_host.h launch_dgrad2 / launch_dgrad3 pass `train_conv_variant() != 0` as the
pipelined flag) and wgrad_variant (30, 2: csrc/wgrad_mfma.hip wgrad_variant()) leave no trace: their runs hold the alternative
kernels to the same stage criteria.

x is bf16-representable in both feature dtypes (except under folded jitter, where block 1 reads fp32), so the stage statements
need not know whether a kernel rounds its input.

Measured on an MI355X (this file: 51 tests, 18 s; the largest case, [2,321,180] with its CPU oracle, 1.2 s -- [2,323,180] takes
the same, so both stay in CASES).  Worst over the 14 default bf16 runs, per stage family.  bf16 tensors: the largest element
deviation as a share of its allowance 2^-8 |want| + K u A, the share of K u A in use beyond half a bf16 step, the largest unequal
share of any one tensor (the cap is on the case's pooled share: 0 .. 7.4e-05 measured, cap 1e-3).  fp32 outputs: the tensor
closest to its bound.

  stage family                          tensors  worst deviation                                              bound
  block 1 forward a1                       14    1.00 of allowance, 0.01 of K u A; unequal 9.5e-05            1
  conv3x3 forward z2, z3                   28    0.98 of allowance, 0.00 of K u A; unequal 1.8e-04            1
  BatchNorm + ReLU + pool a2               14    1.00 of allowance, 0.01 of K u A; unequal 1.2e-04            1
  BatchNorm backward dz3, dz2              28    1.00 of allowance, 0.04 of K u A; unequal 1.3e-04;           1
                                                 open ReLU decisions 0                                        1e-4
  conv3x3 data gradient da2, da1           28    0.97 of allowance, 0.00 of K u A; unequal 2.8e-04            1
  batch + running statistics              210    b3.var max 3.6e-07, l2 1.3e-07 (floor 1.1e-07)               1.0e-05
  tap moments XX, Xs                       28    b1.XX max 7.7e-08, l2 4.4e-08 (floor 8.6e-07)                1.0e-05
  emb, msum                                42    b3.emb max 2.8e-07, l2 1.1e-07 (floor 7.8e-08); counts exact 1.0e-05
  logits, loss, dlogits                    42    bce.loss 1.5e-06 (floor 1.5e-06)                             1.2e-05
  classifier backward                      42    classifier.weight max 1.0e-07, l2 4.2e-08 (floor 1.0e-07)    1.0e-05
  BatchNorm gamma, beta gradients (2, 3)   56    conv.6.weight max 3.3e-07, l2 2.8e-07 (floor 1.9e-07)        1.0e-05
  conv3x3 weight gradient                  28    conv.5.weight max 4.0e-07, l2 6.8e-07 (floor 6.1e-07)        1.0e-05
  conv3x3 bias gradient                    28    conv.10.bias 6.6e-09 of sum |dz| (floor 6.1e-09)             1.0e-05
  block 1 gradients                        56    conv.1.weight max 3.6e-07 (floor 1.4e-07)                    1.0e-05
  block 1 record A, S1, S2                 35    b1.rec.S2 max 3.6e-07 (floor 1.4e-07)                        1.0e-05
  block 1 open ReLU decisions              14    3.2e-06 at [2,323,180]                                       1e-4

The 5 fp32-precision runs are closest to their bound at da2 [2,321,180]: max 1.9e-06, l2 6.1e-07 against 1.2e-05, 1.0e-05 (floor
1.5e-06).  The 21 option runs, the 6 dropout runs and the 4 augmentation runs give the same picture (fp32 tensor closest to its
bound: b3.msum.sx at [2,321,180] under jitter, max 9.1e-07, floor 2.5e-07); with dropout a1 uses up to 0.91 of its K u A (the
keep-scale is folded into block 1's weights) and the pooled unequal share is 3.4e-05 .. 7.9e-05.
"""
import contextlib
import ctypes as C
import json
import math
import os
import random
import time

import pytest
import torch

import cnn2d_stage_oracle as S
import workspace_bands as WB
from dfa_amd import _lib
from dfa_amd.model import CNN2D
from dfa_amd.training.train_step import backward_raw, forward_train_raw

pytestmark = pytest.mark.gpu

SEED = 7
DEFAULTS = {"conv1_mfma": 1, "conv1_bwd_fused": 1, "dgrad_m16": 1, "train_conv_variant": 2, "wgrad_variant": 3}
OPTION_RUNS = [("conv1_mfma", 0), ("conv1_bwd_fused", 0), ("dgrad_m16", 0), ("train_conv_variant", 0), ("train_conv_variant", 1),
               ("wgrad_variant", 30), ("wgrad_variant", 2)]
OPTION_SHAPES = [(2, 7, 31), (3, 21, 65), (2, 321, 180)]
FP32_SHAPES = [(1, 4, 5), (2, 7, 31), (2, 10, 33), (3, 21, 65), (2, 321, 180)]
AUG_SHAPES = [(3, 21, 65), (2, 321, 180)]
AUG_CFG = dict(spec_augment=True, time_mask_ratio=0.2, feature_mask=True, feature_mask_ratio=0.1, time_shift=True, time_shift_ratio=0.1,
               channel_drop=True, channel_drop_prob=0.3, gaussian_jitter_std=0.05)
ACT = {"a1": ("H1", 32), "z2": ("H1", 64), "a2": ("H2", 64), "z3": ("H2", 128), "dz3": ("H2", 128), "da2": ("H2", 64), "dz2": ("H1", 64),
       "da1": ("H1", 32)}


@pytest.fixture
def option():
    """set one option for a test; every option this file touches is back at its default afterwards (the two variants are
    process-wide)"""
    ctx = _lib.Context.get(torch.device("cuda", 0))

    @contextlib.contextmanager
    def with_(name=None, value=0):
        try:
            if name is not None:
                ctx.set_option(name, value)
            yield
        finally:
            for n, v in DEFAULTS.items():
                ctx.set_option(n, v)
    return with_


def _region(ws, off, shape, dtype):
    n = math.prod(shape) * torch.empty((), dtype=dtype).element_size()
    return ws[off:off + n].view(dtype).reshape(shape)


def run_step(shape, x_dtype, prec="bf16", p=0.0, jitter=None):
    """one training step -> (state dict before the step, plan, operands as float64 CPU tensors, the model)"""
    B, T, F = shape
    dev = torch.device("cuda", 0)
    sd = S.ordinary_state(SEED, F)
    model = CNN2D(in_features=F, dropout=p, precision=prec)
    model.load_state_dict(sd)
    model = model.to(dev).train()
    model._drop_seed = 77
    xb, y = S.case_input(B, T, F)
    # bf16 features: the strided [B, T, F] view of [B, F, T] storage the loaders hand over; fp32 features: [B, T, F] storage
    x = xb.to(torch.bfloat16).transpose(1, 2).contiguous().to(dev).transpose(1, 2) if x_dtype == torch.bfloat16 else xb.to(dev)
    x_seen = xb
    ctx = _lib.Context.get(dev)
    code = _lib.PRECISIONS[prec]
    pl = _lib.cnn2d_train_plan(ctx.handle, B, T, F, code)
    assert pl.total == ctx.lib.dfa_cnn2d_train_workspace_bytes(ctx.handle, B, T, F, code) and pl.elem == (2 if prec == "bf16" else 4)
    if jitter is not None:        # the stand-alone pass with the same seeds gives the x the block-1 stages read
        from dfa_amd.augmentation import FusedAugment
        cfg = dict(AUG_CFG, gaussian_jitter=jitter)
        random.seed(41); torch.manual_seed(41)
        x_seen = FusedAugment(seed=5, fold=False, out_dtype=torch.float32, **cfg)(x).float().cpu()
        random.seed(41); torch.manual_seed(41)
        FusedAugment(seed=5, fold=True, **cfg)(x)                 # arms the same draw for the next forward
    ws, check_bands = WB.banded(pl.total, device=dev)     # exactly the plan's bytes, 0xFF (NaN as bf16 and as fp32), between canary bands
    model._train_ws = ws
    (logits,), st = forward_train_raw(model, x)
    assert st.ws is ws, "the library replaced the injected workspace: its planner asked for more than the plan's total"
    yd = y.to(dev)
    loss = torch.full((1,), float("nan"), device=dev)
    dlogits = torch.full((B,), float("nan"), device=dev)
    _lib.check(ctx.handle, ctx.lib.dfa_bce_smooth_fwd_bwd(ctx.handle, C.c_void_p(logits.data_ptr()), C.c_void_p(yd.data_ptr()), S.SMOOTHING, B,
                                                          C.c_void_p(loss.data_ptr()), C.c_void_p(dlogits.data_ptr())))
    grads = [torch.full(q.shape, float("nan"), dtype=torch.float32, device=dev) for q in model.parameters()]
    names = [n for n, _ in model.named_parameters()]
    assert names == S.PARAM_ORDER
    backward_raw(model, x, dlogits, grads, st)
    check_bands(f"cnn2d training step {list(shape)}")
    et, f32 = (torch.bfloat16 if prec == "bf16" else torch.float32), torch.float32
    o = {"x": x_seen.to(S.F64), "y": y.to(S.F64), "p": p, "keep": [1.0, 1.0], "logits": logits.reshape(B).cpu().to(S.F64), "loss": float(loss),
         "dlogits": dlogits.cpu().to(S.F64), "grads": {n: g.cpu().to(S.F64) for n, g in zip(names, grads)}}
    for k, (h, c) in ACT.items():
        o[k] = _region(ws, getattr(pl, k), (B, getattr(pl, h), F, c), et).cpu().to(S.F64)
    o["emb"] = _region(ws, pl.emb, (B, 128, F), f32).cpu().to(S.F64)
    o["demb"] = _region(ws, pl.demb, (B, F, 128), f32).cpu().to(S.F64)
    o["msum"] = _region(ws, pl.msum, (B, F, 128, 2), f32).cpu().to(S.F64)
    stats = _region(ws, pl.stats, (3 * sum(S.BN_C),), f32).cpu().to(S.F64)
    sums = _region(ws, pl.sums, (2 * sum(S.BN_C) + 32 * 11 + 90,), f32).cpu().to(S.F64)
    off = 0
    o["mean"], o["var"], o["invstd"], o["sums"] = [], [], [], []
    for c in S.BN_C:         # mean | var | invstd and (S1, S2) per layer, the layers behind each other (include/dfa_hip.h)
        blk = stats[3 * off:3 * (off + c)]
        o["mean"].append(blk[:c]); o["var"].append(blk[c:2 * c]); o["invstd"].append(blk[2 * c:])
        o["sums"].append(sums[2 * off:2 * (off + c)].reshape(c, 2))
        off += c
    o["c1rec"] = sums[2 * off:2 * off + 352].reshape(32, 11)
    o["XX"], o["Xs"] = sums[2 * off + 352:2 * off + 433].reshape(9, 9), sums[2 * off + 433:2 * off + 442]
    o["raw"] = _region(ws, pl.raw, (B, pl.H2, F, 64), f32).cpu()
    bns = [model.conv[i] for i in model._BN_IDX]
    o["run"] = [(bn.running_mean.cpu().to(S.F64), bn.running_var.cpu().to(S.F64)) for bn in bns]
    assert all(int(bn.num_batches_tracked) == int(sd[f"{n}.num_batches_tracked"]) + 1 for bn, n in zip(bns, S.BNL))
    return sd, pl, o, model


def check_step(shape, x_dtype, tag, prec="bf16", p=0.0, jitter=None, opt=(None, 0)):
    B, T, F = shape
    t0 = time.time()
    sd, pl, o, model = run_step(shape, x_dtype, prec, p, jitter)
    name, value = opt
    # ---- the path the options select (csrc/train_api.hip: train_c1_fused, train_c1_mfma, train_dgrad_m16) ...
    m16 = prec == "bf16" and not (name == "dgrad_m16" and value == 0)
    fused = name != "conv1_bwd_fused"
    mfma = (fused and name != "conv1_mfma" and prec == "bf16" and x_dtype == torch.bfloat16 and jitter is None and F <= 224
            and (p == 0 or m16))
    # ---- ... and what it leaves in the NaN-filled workspace
    assert bool(torch.isnan(o["raw"]).all()) == m16, ("raw is written exactly by the two-launch data gradient", name)
    assert bool(torch.isfinite(o["raw"]).all()) != m16
    for key in ("XX", "Xs"):
        assert bool(torch.isfinite(o[key]).all()) == fused and bool(torch.isnan(o[key]).all()) != fused, (key, name)
    rec = o["c1rec"].reshape(-1)
    assert bool(torch.isfinite(rec[:320]).all()), "block 1's backward record"
    assert bool(torch.isfinite(rec[320:]).all()) == fused and bool(torch.isnan(rec[320:]).all()) != fused, "[32][11] on the one-pass backward, [32][10] on the two-pass one"
    assert bool(torch.isfinite(o["sums"][0]).all()) != fused, "layer 1's (S1, S2) record is the two-pass backward's"
    if fused:
        assert bool((o["c1rec"][:, 10] == 0).all()) == mfma, "S2 is left 0 (and derived) exactly by the matrix-core pass"
    else:           # the two-pass record is dW[9] | db per channel, and the layer's sums are its BatchNorm gradients: all bit for bit
        rec = rec[:320].reshape(32, 10)
        assert torch.equal(rec[:, :9], o["grads"]["conv.0.weight"].reshape(32, 9)) and torch.equal(rec[:, 9], o["grads"]["conv.0.bias"])
        assert torch.equal(o["sums"][0][:, 0], o["grads"]["conv.1.bias"]) and torch.equal(o["sums"][0][:, 1], o["grads"]["conv.1.weight"])
        o["c1rec"] = o["XX"] = o["Xs"] = None
    # ---- every stored tensor is finite (a NaN left in a region is an element no kernel wrote)
    for key in list(ACT) + ["emb", "demb", "msum", "logits", "dlogits"]:
        assert bool(torch.isfinite(o[key]).all()), (key, "not finite")
    assert all(bool(torch.isfinite(t).all()) for key in ("mean", "var", "invstd") for t in o[key])
    assert all(bool(torch.isfinite(g).all()) for g in o["grads"].values()) and math.isfinite(o["loss"])
    # ---- the (S1, S2) records of layers 2 and 3 are the returned gradients, bit for bit
    for l, bn in ((1, "conv.6"), (2, "conv.11")):
        assert torch.equal(o["sums"][l][:, 0], o["grads"][bn + ".bias"]) and torch.equal(o["sums"][l][:, 1], o["grads"][bn + ".weight"]), bn
    # ---- dropout: the keep masks, read off the stored tensors
    if p > 0:
        keeps, det = S.read_keeps(o, sd, p)
        o["keep"], o["det"] = [k.to(S.F64) for k in keeps], det
        for k, d in zip(keeps, det):
            n = int(d.sum())
            share = float(k[d].double().mean())
            # (csrc/rng.h compares 16-bit uniforms with the top 16 bits of p 2^32: the rate is p to within 2^-16)
            assert abs(share - (1 - p)) < 5 * math.sqrt(p * (1 - p) / n) + 2.0 ** -16, ("kept share", share, n)
        dropped1 = ~keeps[0]
        assert bool((o["da1"][dropped1] == 0).all()) == mfma, "da1 is stored masked exactly when the matrix-core block 1 ran"
    # ---- the stages
    kw = dict(elem=prec, fused=fused, da1_masked=mfma and p > 0, s2_derived=mfma)
    want = S.stage_results(o, sd, S.F64, True, **kw)
    floor = S.stage_results(o, sd, S.F32, False, **kw)
    rows, bad, read = S.compare(want, lambda n: S.stored_of(o, n), floor)
    S.print_rows(f"{tag} {time.time() - t0:.1f} s", rows)
    assert not bad, "\n".join(bad)
    # every stored tensor was read by a stage
    must = set(S.PARAM_ORDER) | set(S.STORED) | {"b3.msum.n", "b3.msum.sx", "bce.loss"}
    must |= {f"b{l}.{k}" for l in (1, 2, 3) for k in ("mean", "var", "invstd", "running_mean", "running_var")}
    must |= {"b1.rec.A", "b1.rec.S1"} | (set() if mfma else {"b1.rec.S2"})
    if not fused:
        must -= {"b1.XX", "b1.Xs", "b1.rec.A", "b1.rec.S1", "b1.rec.S2"}
    assert set(read) == must, (sorted(must - set(read)), sorted(set(read) - must))
    return rows


@pytest.mark.parametrize("x_dtype", [torch.bfloat16, torch.float32], ids=["xbf16", "xfp32"])
@pytest.mark.parametrize("shape", S.CASES, ids=str)
def test_every_stage_on_the_gpus_own_operands(shape, x_dtype, option):
    """default bf16 runs: x in bf16 (matrix-core block 1) and in fp32 (vector block 1)"""
    with option():
        check_step(shape, x_dtype, f"cnn2d stages {list(shape)} {'xbf16' if x_dtype == torch.bfloat16 else 'xfp32'}")


@pytest.mark.parametrize("shape", FP32_SHAPES, ids=str)
def test_every_stage_in_fp32_precision(shape, option):
    """ordinary state, element-wise ReLU masks, a dropped row under a live mask: what the saturated-state tests cannot give"""
    with option():
        check_step(shape, torch.float32, f"cnn2d stages {list(shape)} fp32", prec="fp32")


@pytest.mark.parametrize("opt", OPTION_RUNS, ids=lambda o: f"{o[0]}={o[1]}")
@pytest.mark.parametrize("shape", OPTION_SHAPES, ids=str)
def test_every_stage_with_one_option_changed(shape, opt, option):
    with option(*opt):
        check_step(shape, torch.bfloat16, f"cnn2d stages {list(shape)} {opt[0]}={opt[1]}", opt=opt)


@pytest.mark.parametrize("mfma", [1, 0], ids=["conv1_mfma", "conv1_vector"])
@pytest.mark.parametrize("shape", OPTION_SHAPES, ids=str)
def test_every_stage_with_dropout(shape, mfma, option):
    """p = 0.3: the keep masks are read off the stored a1 / a2, the backward stages are evaluated with them"""
    with option("conv1_mfma", mfma):
        check_step(shape, torch.bfloat16, f"cnn2d stages {list(shape)} p=0.3 conv1_mfma={mfma}", p=0.3, opt=(None if mfma else "conv1_mfma", 0))


@pytest.mark.parametrize("jitter", [False, True], ids=["masks_roll_drop", "jitter"])
@pytest.mark.parametrize("shape", AUG_SHAPES, ids=str)
def test_every_stage_with_folded_augmentation(shape, jitter, option):
    with option():
        check_step(shape, torch.bfloat16, f"cnn2d stages {list(shape)} augment jitter={jitter}", jitter=jitter)


def test_train_plan_refuses_in_the_steps_own_words():
    """a precision or shape dfa_cnn2d_forward_train refuses is refused by dfa_cnn2d_train_plan with the same code and message (the
    messages recorded for the step in tests/golden/abi_train_errors.json)"""
    golden = {name: (code, msg) for name, code, msg in
              json.load(open(os.path.join(os.path.dirname(__file__), "golden", "abi_train_errors.json")))}
    ctx = _lib.Context.get(torch.device("cuda", 0))
    for name, args in (("precision", (2, 8, 20, 3)), ("batch_0", (0, 8, 20, _lib.PREC_BF16)), ("T_short", (2, 3, 20, _lib.PREC_BF16))):
        code, msg = golden["cnn2d_forward_train/" + name]
        assert ctx.lib.dfa_cnn2d_train_plan(ctx.handle, *args, None, 0) == code
        assert ctx.lib.dfa_last_error(ctx.handle).decode() == msg
