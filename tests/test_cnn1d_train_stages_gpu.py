"""The CNN1D training step, uniform and ragged, kernel stage by kernel stage, on the tensors the GPU itself stored.

One dfa_cnn1d_forward_train[_ragged] + dfa_bce_smooth_fwd_bwd + dfa_cnn1d_backward[_ragged] per case through the C ABI, on a
workspace of the test's own that is exactly the plan's size between canary bands and NaN in every byte beforehand
(tests/workspace_bands.py, handed to the model as model._train_ws); the gradient tensors are NaN beforehand too, and so are the
padding frames of a ragged batch's x.  dfa_cnn1d_train_plan says where every stored tensor lies -- no offset or dimension is
restated here -- and after the step the workspace still holds z1-z3, h1, h2, pooled, dpooled, dz1-dz3, dh1, dh2, the statistics
block, the sums block and, behind the uniform plan, a ragged batch's lengths.  Every stage of tests/cnn1d_stage_oracle.py is then
evaluated in float64 on THOSE operands and compared with what the GPU stored for it, so no error propagates from one kernel into
the check of the next and a ReLU flip in one layer (which holds the whole-step comparisons to 3e-2 of scale) does not enter.

Criteria (everything is fp32): the project's fp32 criterion, tests/cae_stage_oracle.py::compare -- max |got - want| / scale and
relative L2 against float64 within max(1e-5, 8 floor), floor = the CPU's float32 evaluation of the same stage on the same operands
(tests/test_cnn1d_train_stages_cpu.py shows the floor is below 1.25e-6 for all but four named stages).  Open ReLU decisions (a float64 BatchNorm output
within K_BN 2^-24 of its terms of zero) enter a sum's bound with their own magnitude and may take either branch in dz; their share
of a layer is capped at 1e-4.  The bias gradients of the three convolutions (sums that cancel to rounding residue) are measured
against the largest channel sum of |dz|.  Under cnn1d_train_x3 = 3 the five convolutions get the allowance derived from their
kept products (3.01 * 2^-16 sum |a| |w| + K 2^-24 A, tests/cnn1d_stage_oracle.py) per element and nothing else: neither the floor nor the 1e-5 term applies to them.
Bit-exact: the (S1, S2) records left in `sums` equal the returned dbeta / dgamma; h and dz are exact zeros at every padding frame;
the lengths table is the batch's; num_batches_tracked is incremented.  The workspace: every region that holds a stored tensor is
finite (z and dh at padding frames included: nothing reads them, but the region was NaN) and is read by a stage (the set of names
is asserted, all 14 gradients among them); the bands are intact; the library did not replace the workspace.
Dropout: the keep masks are read off the stored h1 / h2; the kept share of the determined elements lies within 5 sigma + 2^-16 of
1 - p; the backward stages are evaluated with the masks read, so a backward that regenerates another layer's mask, forgets the
keep-scale or indexes the draw otherwise than the forward fails l*.dz and the BatchNorm gradients.
Folded augmentation: the stand-alone dfa_augment_batch pass with the same seeds gives the x the two layer-1 stages read.

Cases: S.CASES (11 uniform shapes, each the smallest that crosses one boundary of the kernels; none proved degenerate for
BatchNorm, [1,3,20] with its three frames included) and S.RAGGED (sets A-D of tests/test_cnn1d_ragged_train_gpu.py; A, C, D at
F = 20, B at F = 180).

Measured on an MI355X (this file: 40 tests, 3.3 s; the largest case, [2,321,180] with its CPU oracle, 0.04 s).  Worst over the 15
default runs, per stage family: the tensor closest to its bound.

  stage family                          tensors  worst deviation                                                   bound
  Conv1d forward z1-z3                     45    l1.z set B: max 7.3e-07, l2 3.6e-07 (floor 1.5e-07)               1.0e-05
  batch + running statistics              225    l1.mean [2,257,20]: max 8.2e-07, l2 4.6e-07 (floor 1.4e-07)       1.0e-05
  BatchNorm + ReLU + dropout h1, h2        30    l1.h [1,385,20]: max 1.1e-07, l2 4.3e-08 (floor 7.3e-08)          1.0e-05
  pooled                                   15    pooled [1,3,20]: max 2.3e-07, l2 6.8e-08 (floor 5.4e-07)          1.0e-05
  logits, loss, dlogits                    45    bce.loss [2,257,20]: 1.4e-06 (floor 1.4e-06)                      1.1e-05
  classifier backward                      45    classifier.bias [70,5,20]: 1.7e-07 (floor 2.9e-08)                1.0e-05
  BatchNorm gamma, beta gradients          90    conv.5.weight [2,321,180]: max 5.8e-07, l2 3.9e-07 (floor 6.7e-07) 1.0e-05
  BatchNorm backward dz1-dz3               45    l3.dz [1,3,20]: max 2.1e-07, l2 2.6e-07 (floor 2.1e-07)           1.0e-05
  Conv1d weight gradient                   45    conv.8.weight [2,321,180]: max 1.8e-06, l2 1.7e-06 (floor 7.6e-07) 1.0e-05
  Conv1d bias gradient                     45    conv.4.bias [2,321,180]: 1.2e-07 of sum |dz| (floor 4.3e-08)      1.0e-05
  Conv1d data gradient dh2, dh1            30    l3.dx [2,257,20]: max 8.1e-07, l2 3.0e-07 (floor 1.6e-07)         1.0e-05
  open ReLU decisions per layer            45    l3.relu [2,257,20]: 1.5e-05                                       1e-4

The 25 layout, option, dropout, augmentation and hook runs give the same picture (closest: conv.4.weight at [2,321,180] under the
folded masks with option 0, max 3.0e-06 against 1.2e-05, floor 1.5e-06; open decisions 4.9e-05 of layer 1 there).  Under
cnn1d_train_x3 = 3 the five convolutions use 0.015 .. 0.092 of the two-term allowance and would also meet the fp32 criterion at
the three shapes run.  The three-term default fits 8 floor everywhere, so it needs no allowance of its own.
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

import cnn1d_stage_oracle as S
import workspace_bands as WB
from dfa_amd import _lib
from dfa_amd.model_cnn1d import CNN1D
from dfa_amd.training.train_step import backward_raw, forward_train_raw

pytestmark = pytest.mark.gpu

SEED = 7
OPTION_CASES = [(2, 33, 36), (2, 321, 180), "A"]
DROP_CASES = [(2, 321, 180), "A"]
AUG_SHAPES = [(3, 65, 20), (2, 321, 180)]
AUG_CFG = dict(spec_augment=True, time_mask_ratio=0.2, feature_mask=True, feature_mask_ratio=0.1, time_shift=True, time_shift_ratio=0.1,
               channel_drop=True, channel_drop_prob=0.3, gaussian_jitter_std=0.05)


@pytest.fixture
def option():
    """set cnn1d_train_x3 for a test; it is back at its default afterwards (the option is the context's)"""
    ctx = _lib.Context.get(torch.device("cuda", 0))

    @contextlib.contextmanager
    def with_(x3=1):
        try:
            ctx.set_option("cnn1d_train_x3", x3)
            yield
        finally:
            ctx.set_option("cnn1d_train_x3", 1)
    return with_


def _shape(case):
    if isinstance(case, str):
        lengths, T, F = S.RAGGED[case]
        return len(lengths), T, F, lengths
    return (*case, None)


def _f32(ws, off, shape):
    return ws[off:off + 4 * math.prod(shape)].view(torch.float32).reshape(shape).cpu().to(S.F64)


def run_step(case, layout="stored", p=0.0, jitter=None, hook=False):
    """one training step -> (state dict before the step, plan, operands as float64 CPU tensors)"""
    B, T, F, lengths = _shape(case)
    dev = torch.device("cuda", 0)
    sd = S.ordinary_state(SEED, F)
    model = CNN1D(in_features=F, dropout=p)
    model.load_state_dict(sd)
    model = model.to(dev).train()
    model._drop_seed = 77
    stored, y = S.case_input(B, T, F, lengths)                  # [B, F, T], NaN at every padding frame
    x = stored.to(dev).transpose(1, 2)                          # the [B, T, F] view of the stored layout
    if layout == "btf":
        x = x.contiguous()
    x_seen = stored
    ctx = _lib.Context.get(dev)
    pl = _lib.cnn1d_train_plan(ctx.handle, B, T, F, lengths is not None)
    nbytes = ctx.lib.dfa_cnn1d_train_ragged_workspace_bytes if lengths is not None else ctx.lib.dfa_cnn1d_train_workspace_bytes
    assert pl.total == nbytes(ctx.handle, B, T, F)
    if jitter is not None:        # the stand-alone pass with the same seeds gives the x the layer-1 stages read
        from dfa_amd.augmentation import FusedAugment
        cfg = dict(AUG_CFG, gaussian_jitter=jitter)
        random.seed(41); torch.manual_seed(41)
        x_seen = FusedAugment(seed=5, fold=False, out_dtype=torch.float32, **cfg)(x).float().cpu().transpose(1, 2)
        random.seed(41); torch.manual_seed(41)
        FusedAugment(seed=5, fold="cnn1d", **cfg)(x)              # arms the same draw for the next forward
    ws, check_bands = WB.banded(pl.total, device=dev)     # exactly the plan's bytes, 0xFF (NaN as fp32), between canary bands
    model._train_ws = ws
    calls = []
    fn = _lib.BnSync.FN(lambda user, buf, count: calls.append(count) or 0)       # a single-rank identity SyncBN hook: the sums stay the rank's own
    hook_buf = torch.zeros(1024, dtype=torch.float32, device=dev)
    if hook:
        _lib.check(ctx.handle, ctx.lib.dfa_ctx_set_bn_sync(ctx.handle, C.cast(fn, C.c_void_p), None, 1, C.c_void_p(hook_buf.data_ptr()), hook_buf.numel()))
    try:
        (logits,), st = forward_train_raw(model, x, lengths=lengths)
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
        check_bands(f"cnn1d training step {case}")
        # (sum z, sum z^2) of each layer in the forward, (S1, S2) of each layer in the backward: six exchanges of 2 C floats
        assert calls == ([2 * c for c in S.BN_C] + [2 * c for c in reversed(S.BN_C)] if hook else []), calls
    finally:
        if hook:
            _lib.check(ctx.handle, ctx.lib.dfa_ctx_set_bn_sync(ctx.handle, None, None, 1, None, 0))
    o = S.new_operands(x_seen, y, lengths, p)
    o.update(logits=logits.reshape(B).cpu().to(S.F64), loss=float(loss), dlogits=dlogits.cpu().to(S.F64),
             grads={n: g.cpu().to(S.F64) for n, g in zip(names, grads)})
    for key, cs in (("z", S.BN_C), ("h", S.BN_C[:2]), ("dz", S.BN_C), ("dh", S.BN_C[:2])):
        o[key] = [_f32(ws, getattr(pl, key)[l], (B, c, T)) for l, c in enumerate(cs)]
    o["pooled"], o["dpooled"] = _f32(ws, pl.pooled, (B, 128)), _f32(ws, pl.dpooled, (B, 128))
    stats, sums = _f32(ws, pl.stats, (3 * sum(S.BN_C),)), _f32(ws, pl.sums, (2 * sum(S.BN_C),))
    off = 0
    o["sums"] = []
    for l, c in enumerate(S.BN_C):         # mean | var | invstd and (S1, S2) per layer, the layers behind each other (include/dfa_hip.h)
        blk = stats[3 * off:3 * (off + c)]
        o["mean"][l], o["var"][l], o["invstd"][l] = blk[:c], blk[c:2 * c], blk[2 * c:]
        o["sums"].append(sums[2 * off:2 * (off + c)].reshape(c, 2))
        off += c
    if lengths is not None:
        assert ws[pl.lengths:pl.lengths + 4 * B].view(torch.int32).cpu().tolist() == lengths, "the lengths table behind the uniform plan"
    else:
        assert pl.lengths == -1
    bns = [model.conv[i] for i in model._BN_IDX]
    o["run"] = [(bn.running_mean.cpu().to(S.F64), bn.running_var.cpu().to(S.F64)) for bn in bns]
    assert all(int(bn.num_batches_tracked) == int(sd[f"{n}.num_batches_tracked"]) + 1 for bn, n in zip(bns, S.BNL))
    return sd, pl, o


def evaluate(o, sd, x3=1):
    """every stage on the operand set -> (rows, failures, the names of the stages that read a stored tensor)"""
    p = o["p"]
    bad = []
    if p > 0:         # dropout: the keep masks, read off the stored tensors
        keeps, det = S.read_keeps(o, sd)
        o["keep"], o["det"] = [k.to(S.F64) for k in keeps], det
        bad += S.kept_share_failures(keeps, det, p)
    want = S.stage_results(o, sd, S.F64, True, conv_terms=2 if x3 == 3 else 3)
    floor = S.stage_results(o, sd, S.F32, False)
    rows, worse, read = S.compare(want, lambda n: S.stored_of(o, n), floor)
    return rows, bad + worse + S.padding_failures(o), read


def check_step(case, tag, x3=1, **kw):
    t0 = time.time()
    sd, pl, o = run_step(case, **kw)
    # ---- every stored tensor is finite (a NaN left in a region is an element no kernel wrote)
    for key in ("z", "h", "dz", "dh", "mean", "var", "invstd", "sums"):
        assert all(bool(torch.isfinite(t).all()) for t in o[key]), (key, "not finite")
    for key in ("pooled", "dpooled", "logits", "dlogits"):
        assert bool(torch.isfinite(o[key]).all()), (key, "not finite")
    assert all(bool(torch.isfinite(g).all()) for g in o["grads"].values()) and math.isfinite(o["loss"])
    # ---- the (S1, S2) records are the returned gradients, bit for bit
    for l, bn in enumerate(S.BNL):
        assert torch.equal(o["sums"][l][:, 0], o["grads"][bn + ".bias"]) and torch.equal(o["sums"][l][:, 1], o["grads"][bn + ".weight"]), bn
    rows, bad, read = evaluate(o, sd, x3)
    S.print_rows(f"{tag} {time.time() - t0:.1f} s", rows)
    assert not bad, "\n".join(bad)
    assert set(read) == S.stage_names() and set(S.PARAM_ORDER) <= set(read), sorted(S.stage_names() ^ set(read))
    return rows


@pytest.mark.parametrize("shape", S.CASES, ids=str)
def test_every_stage_on_the_gpus_own_operands(shape, option):
    with option():
        check_step(shape, f"cnn1d stages {list(shape)}")


@pytest.mark.parametrize("name", list(S.RAGGED))
def test_every_stage_of_a_ragged_batch(name, option):
    with option():
        check_step(name, f"cnn1d stages ragged {name}")


@pytest.mark.parametrize("case", [(2, 33, 36), "A"], ids=str)
def test_every_stage_on_a_contiguous_btf_batch(case, option):
    """x contiguous as [B, T, F]: frames are not contiguous, the layer-1 convolution and weight gradient take the strided loads"""
    with option():
        check_step(case, f"cnn1d stages {case} btf", layout="btf")


@pytest.mark.parametrize("x3", [0, 2, 3])
@pytest.mark.parametrize("case", OPTION_CASES, ids=str)
def test_every_stage_under_every_x3_option(case, x3, option):
    """0: the fp32 vector-ALU convolutions and the fp32 matrix-core weight gradient; 2: one channel tile per workgroup; 3: two bf16
    terms per operand, held to the allowance derived from the kept products"""
    with option(x3):
        check_step(case, f"cnn1d stages {case} x3={x3}", x3=x3)


@pytest.mark.parametrize("x3", [1, 0])
@pytest.mark.parametrize("case", DROP_CASES, ids=str)
def test_every_stage_with_dropout(case, x3, option):
    """p = 0.3: the keep masks are read off the stored h1 / h2, the backward stages are evaluated with them"""
    with option(x3):
        check_step(case, f"cnn1d stages {case} p=0.3 x3={x3}", x3=x3, p=0.3)


@pytest.mark.parametrize("x3", [1, 0])
@pytest.mark.parametrize("jitter", [False, True], ids=["masks_roll_drop", "jitter"])
@pytest.mark.parametrize("shape", AUG_SHAPES, ids=str)
def test_every_stage_with_folded_augmentation(shape, jitter, x3, option):
    with option(x3):
        check_step(shape, f"cnn1d stages {list(shape)} augment jitter={jitter} x3={x3}", x3=x3, jitter=jitter)


def test_every_stage_under_a_single_rank_syncbn_hook(option):
    """the unshifted statistics path and bn_sync_sums"""
    with option():
        check_step((2, 33, 36), "cnn1d stages [2, 33, 36] SyncBN hook", hook=True)


def test_train_plan_refuses_in_the_steps_own_words():
    """a shape dfa_cnn1d_forward_train[_ragged] refuses is refused by dfa_cnn1d_train_plan with the same code and message (the
    messages recorded for the step in tests/golden/abi_train_errors.json)"""
    golden = {name: (code, msg) for name, code, msg in
              json.load(open(os.path.join(os.path.dirname(__file__), "golden", "abi_train_errors.json")))}
    ctx = _lib.Context.get(torch.device("cuda", 0))
    for name, args in (("cnn1d_forward_train/batch_0", (0, 8, 20, 0)), ("cnn1d_forward_train/T_0", (2, 0, 20, 0)),
                       ("cnn1d_forward_train_ragged/batch_0", (0, 8, 20, 1)), ("cnn1d_forward_train_ragged/T_0", (2, 0, 20, 1)),
                       ("cnn1d_forward_train_ragged/T_short", (2, 2, 20, 1)), ("cnn1d_train_plan/F_0", (2, 8, 0, 0))):
        code, msg = golden[name]
        assert ctx.lib.dfa_cnn1d_train_plan(ctx.handle, *args, None, 0) == code, name
        assert ctx.lib.dfa_last_error(ctx.handle).decode() == msg, name
