"""The ConvAutoencoder's bf16 training step, kernel stage by kernel stage, on the tensors the GPU itself stored.

One dfa_cae_forward_train + dfa_cae_backward per case through the C ABI, on a workspace of the test's own that is NaN in every
byte beforehand (handed to the model the way tests/workspace_bands.py does).  dfa_cae_train_plan says where every stored tensor
lies -- no offset or dimension is restated here -- and after the step the workspace still holds e, z, zd, d, dd, de, dz, the
statistics and (option cae_bwd_fold = 0) dzd.  Every stage of tests/cae_stage_oracle.py is then evaluated in float64 on THOSE
operands and compared with what the GPU stored for it, so no error propagates from one kernel into the check of the next and the
conditioning of the network (which holds a whole-step comparison in this mode to 10-20 %) does not enter.

Criteria (tests/cae_stage_oracle.py::compare; tests/test_cae_train_stages_cpu.py shows the CPU's float32 stages meet each with an
eighth of its cap):
  tensors stored in bf16   every element |got - want| <= 2^-8 |want| + K 2^-24 A (half a bf16 step + the rigorous bound of an fp32
                           evaluation of the element's K terms of total magnitude A); at most 1e-3 of a case's elements not
                           bit-equal to bf16(want); a BatchNorm-backward element whose float64 BatchNorm output lies within the
                           fp32 rounding of its own terms of zero may take either ReLU branch, at most 1e-4 of a tensor may be
                           such.
  fp32 outputs             (30 gradients, statistics, reconstruction, MSE) max |got - want| / scale and relative L2 against
                           float64 within max(1e-5, 8 floor), floor = the CPU's float32 evaluation of the same stage on the same
                           operands.  1e-5 lies a hundred times under one missing pixel of the largest case.  Open ReLU
                           decisions enter a sum's bound with their own magnitude.  encoder.0.bias (a sum that cancels to
                           rounding noise, formed from a tensor that is never stored) is measured against the largest channel sum
                           of |dz|.
  the workspace            every region that holds a stored tensor is finite and is read by a stage; the weight matrices left
                           in wq / dwq are the last layer's, bit for bit.  (raw, sums, rec and partial are scratch that is
                           consumed inside the step: what passes through them is checked at the gradients and statistics they
                           end in, not in place.)  The workspace is exactly the plan's size between canary bands.
With the folded BatchNorm-backward pass (the default) dzd is never stored: decoder block 1's is read back from the patch-major
copy in zp; blocks 2 and 3 are restated as bf16(float64 dzd) and their consumers (data gradient, weight and bias gradient) carry
the allowance of that restatement through their own sums.  The run with cae_bwd_fold = 0 reads all three directly.

x is bf16-representable in both feature dtypes (bf16 features: the matrix-core block 1; fp32 features: the vector path), so the
stage statements need not know whether a kernel rounds its input.

Options: which kernel an option selects is not reported by the library for the training step.  Two options leave a trace in the
NaN-filled workspace and are asserted in EVERY run: cae_bwd_fold (dzd written only when 0) and cae_dgrad_mfma (the fp32 GEMM
scratch xf written only when 0).  cae_conv_stats = 0 changes what the statistics stage states (sums of the stored tensor).  For
cae_enc4_wide, dgrad_m16, conv1_mfma and cae_enc1_mfma the dispatch was confirmed by reading cae_train_api.hip (the flags are
read at lines that select the launcher); their runs hold the alternative kernels to the same stage criteria.

Measured on an MI355X (this file: 38 tests, 11 s; the largest case 1.1 s).  Worst over the 16 default runs and the three
cae_bwd_fold = 0 runs, per stage family.  bf16 tensors: the largest element deviation as a share of its allowance
2^-8 |want| + K u A, the share of K u A in use beyond half a bf16 step, the largest unequal share of any one tensor (the cap is on
the case's pooled share: 1.1e-5 .. 7.4e-5 measured, cap 1e-3).  fp32 outputs: the tensor closest to its bound.

  stage                               tensors  worst deviation                                              bound
  block 1 forward e[0]                   19    0.99 of allowance, 0.00 of K u A; unequal 2.6e-05            1
  conv3x3 forward z                      57    0.97 of allowance, 0.00 of K u A; unequal 2.4e-04            1
  ConvTranspose2d forward zd             57    0.99 of allowance, 0.00 of K u A; unequal 9.8e-04 (1 of 1024) 1
  BatchNorm + ReLU (+ pool) e, d        114    1.00 of allowance, 0.03 of K u A; unequal 2.2e-04            1
  decoder 4 backward dd[2]               19    0.99 of allowance, 0.02 of K u A; unequal 3.9e-04            1
  BatchNorm backward dz, dzd             82    1.00 of allowance, 0.04 of K u A; unequal 4.3e-04;           1
                                               open ReLU decisions 1.6e-05                                  1e-4
  conv3x3 data gradient de               57    0.96 of allowance, 0.00 of K u A; unequal 5.9e-04            1
  ConvTranspose2d data gradient          57    0.99 of allowance, 0.00 of K u A; unequal 3.4e-04            1
  batch statistics (mean, var, invstd)  399    enc2.var max 8.2e-07, l2 2.5e-07 (floor 1.3e-07)             1.0e-05
  reconstruction, MSE                    38    dec4.recon max 1.7e-07, l2 7.8e-08 (floor 1.7e-07)           1.0e-05
  decoder.9 weight, bias gradient        38    decoder.9.weight max 1.2e-07, l2 6.6e-08 (floor 2.5e-07)     1.0e-05
  BatchNorm gamma, beta gradients       228    encoder.5.weight max 3.9e-07, l2 1.8e-07 (floor 2.0e-07)     1.0e-05
  ConvTranspose2d weight gradient        57    decoder.6.weight max 9.2e-08, l2 3.0e-08 (floor 1.5e-07)     1.0e-05
  ConvTranspose2d bias gradient          57    decoder.3.bias max 7.5e-06, l2 4.8e-06 (floor 1.9e-06)       1.5e-05, 1.0e-05
  conv3x3 weight gradient                57    encoder.4.weight max 7.9e-07, l2 1.0e-06 (floor 1.4e-06)     1.1e-05, 1.0e-05
  conv3x3 bias gradient                  57    encoder.8.bias max 1.6e-05, l2 7.3e-06 (floor 7.9e-06)       6.3e-05, 2.8e-05
  block 1 gradients                      76    encoder.1.bias max 2.9e-07 (floor 8.2e-07)                   1.0e-05
  block 1 open ReLU decisions            19    4.6e-06 at [2,321,180]                                       1e-4

The bias gradients are sums that cancel to the rounding residue of their bf16 terms, hence their larger floors.  Over the 21 option
runs the picture is the same; the fp32 tensor closest to its bound there is decoder.0.bias at [2,321,180] with cae_bwd_fold = 0
(max 7.3e-05 against 1.8e-04, floor 2.2e-05).
"""
import contextlib
import math

import pytest
import torch

import cae_stage_oracle as S
import workspace_bands as WB
from dfa_amd import _lib
from dfa_amd.model_cae import ConvAutoencoder
from dfa_amd.training.train_step import backward_raw, forward_train_raw

pytestmark = pytest.mark.gpu

SEED = 7
OPTIONS = ("cae_enc4_wide", "dgrad_m16", "cae_dgrad_mfma", "cae_conv_stats", "cae_bwd_fold", "conv1_mfma", "cae_enc1_mfma")
OPTION_SHAPES = [(2, 17, 20), (3, 31, 36), (2, 321, 180)]


@pytest.fixture
def option():
    """set one context option to 0 for a test; every option this file touches is back at its default (1) afterwards"""
    ctx = _lib.Context.get(torch.device("cuda", 0))

    @contextlib.contextmanager
    def off(name):
        if name is not None:
            ctx.set_option(name, 0)
        try:
            yield
        finally:
            for n in OPTIONS:
                ctx.set_option(n, 1)
    return off


def _region(ws, off, shape, dtype):
    n = math.prod(shape) * torch.empty((), dtype=dtype).element_size()
    return ws[off:off + n].view(dtype).reshape(shape)


def run_step(shape, x_dtype):
    """one bf16 training step -> (state, plan, operands as float64 CPU tensors, the raw workspace)"""
    B, T, F = shape
    dev = torch.device("cuda", 0)
    sd = S.ordinary_state(SEED)
    model = ConvAutoencoder(precision="bf16")
    model.load_state_dict(sd)
    model = model.to(dev).train()
    xb = S.case_input(B, T, F).to(torch.bfloat16)
    x = xb.to(dev) if x_dtype == torch.bfloat16 else xb.float().to(dev)
    ctx = _lib.Context.get(dev)
    pl = _lib.cae_train_plan(ctx.handle, B, T, F, _lib.PREC_BF16)
    assert pl.total == ctx.lib.dfa_cae_train_workspace_bytes(ctx.handle, B, T, F, _lib.PREC_BF16) and pl.elem == 2
    ws, check_bands = WB.banded(pl.total, device=dev)     # exactly the plan's bytes, 0xFF (NaN as bf16 and as fp32), between canary bands
    model._train_ws = ws
    (recon, mse), st = forward_train_raw(model, x, want=("recon", "mse"))
    assert st.ws is ws, "the library replaced the injected workspace: its planner asked for more than the plan's total"
    grads = [torch.full(p.shape, float("nan"), dtype=torch.float32, device=dev) for p in model.parameters()]
    names = [n for n, _ in model.named_parameters()]
    assert names == S.PARAM_ORDER
    backward_raw(model, x, None, grads, st)
    check_bands(f"cae training step {list(shape)}")
    bf, f32 = torch.bfloat16, torch.float32

    def act(off, H, W, C):
        return None if off < 0 else _region(ws, off, (B, H, W, C), bf).cpu().to(S.F64)
    o = {"x": xb.to(S.F64), "recon": recon.cpu().to(S.F64), "mse": mse.cpu().to(S.F64),
         "grads": {n: g.cpu().to(S.F64) for n, g in zip(names, grads)}}
    o["e"] = [act(pl.e[l], pl.H[l + 1], pl.W[l + 1], pl.C[l]) for l in range(4)]
    o["de"] = [act(pl.de[l], pl.H[l + 1], pl.W[l + 1], pl.C[l]) for l in range(4)]
    o["z"] = [act(pl.z[l], pl.H[l], pl.W[l], pl.C[l]) for l in range(4)]
    o["dz"] = [act(pl.dz[l], pl.H[l], pl.W[l], pl.C[l]) for l in range(4)]
    for key in ("zd", "d", "dd", "dzd"):
        o[key] = [act(getattr(pl, key)[l], pl.Hd[l], pl.Wd[l], pl.C[4 + l]) for l in range(3)]
    for key in ("mean", "var", "invstd"):
        o[key] = [_region(ws, getattr(pl, key)[i], (pl.C[i],), f32).cpu().to(S.F64) for i in range(7)]
    return sd, pl, o, ws


def check_step(shape, x_dtype, tag, opt=None):
    B, T, F = shape
    sd, pl, o, ws = run_step(shape, x_dtype)
    folded = opt != "cae_bwd_fold"
    # ---- what the options leave in the NaN-filled workspace
    dzd_nan = [bool(torch.isnan(t).all()) for t in o["dzd"]]
    assert dzd_nan == [folded] * 3, ("dzd is written exactly when cae_bwd_fold = 0", dzd_nan, opt)
    Hin, Win, Cin, Cout = pl.Hd[0] // 2, pl.Wd[0] // 2, pl.C[3], pl.C[4]
    xf = _region(ws, pl.xf, (B * Hin * Win * Cin,), torch.float32)
    assert bool(torch.isnan(xf).all()) == (opt != "cae_dgrad_mfma"), ("xf is written exactly when cae_dgrad_mfma = 0", opt)
    # ---- zp holds decoder block 1's dzd patch-major ([pixel][2][2][C]); wq / dwq its weight and weight gradient as [Cin][4 Cout]
    zp = _region(ws, pl.zp, (B, Hin, Win, 2, 2, Cout), torch.bfloat16).cpu().to(S.F64)
    assert bool(torch.isfinite(zp).all())
    dzd0 = zp.permute(0, 1, 3, 2, 4, 5).reshape(B, 2 * Hin, 2 * Win, Cout)
    if folded:
        o["dzd"][0] = dzd0
    else:
        assert torch.equal(o["dzd"][0], dzd0), "zp is not the pixel-unshuffled dzd of decoder block 1"
    w0 = sd["decoder.0.weight"].to(S.F64)                                      # [Cin][Cout][2][2] -> [Cin][q][Cout]
    for region, t in ((pl.wq, w0), (pl.dwq, o["grads"]["decoder.0.weight"].reshape(w0.shape))):
        got = _region(ws, region, (Cin, 4, Cout), torch.float32).cpu().to(S.F64)
        assert torch.equal(got, t.reshape(Cin, Cout, 4).permute(0, 2, 1)), "wq / dwq"
    # ---- every stored tensor is finite (a NaN left in a region is an element no kernel wrote)
    for key in ("e", "de", "z", "dz", "zd", "d", "dd", "mean", "var", "invstd") + (() if folded else ("dzd",)):
        for l, t in enumerate(o[key]):
            assert t is None or bool(torch.isfinite(t).all()), (key, l, "not finite")
    assert all(bool(torch.isfinite(g).all()) for g in o["grads"].values())
    # ---- the stages
    kw = dict(stats="stored" if opt == "cae_conv_stats" else "epilogue", dgrad_bf16=opt != "cae_dgrad_mfma",
              have_dzd=(True, not folded, not folded))
    want = S.stage_results(o, sd, S.F64, True, **kw)
    floor = S.stage_results(o, sd, S.F32, False, **kw)
    rows, bad, read = S.compare(want, lambda name: S.stored_of(o, name), floor)
    S.print_rows(tag, rows)
    assert not bad, "\n".join(bad)
    # every stored tensor was read by a stage: as a result ...
    assert set(S.PARAM_ORDER) <= set(read) and {"dec4.recon", "dec4.mse", "dec4.dd", "enc1.e"} <= set(read)
    for l in range(1, 4):
        assert {f"enc{l + 1}.z", f"enc{l + 1}.e", f"enc{l + 1}.dz", f"enc{l + 1}.dx"} <= set(read)
        assert {f"dec{l}.zd", f"dec{l}.d", f"dec{l}.dx"} <= set(read)
    assert ("dec1.dzd" in read) and (("dec2.dzd" in read and "dec3.dzd" in read) != folded)
    for i in range(7):
        name = f"enc{i + 1}" if i < 4 else f"dec{i - 3}"
        assert {name + ".mean", name + ".var", name + ".invstd"} <= set(read)


@pytest.mark.parametrize("x_dtype", [torch.bfloat16, torch.float32], ids=["xbf16", "xfp32"])
@pytest.mark.parametrize("shape", S.CASES, ids=str)
def test_every_stage_on_the_gpus_own_operands(shape, x_dtype, option):
    with option(None):
        check_step(shape, x_dtype, f"cae stages {list(shape)} {'xbf16' if x_dtype == torch.bfloat16 else 'xfp32'}")


@pytest.mark.parametrize("opt", OPTIONS)
@pytest.mark.parametrize("shape", OPTION_SHAPES, ids=str)
def test_every_stage_with_one_option_off(shape, opt, option):
    with option(opt):
        check_step(shape, torch.bfloat16, f"cae stages {list(shape)} {opt}=0", opt)


def test_train_plan_refuses_in_the_steps_own_words():
    """a precision or shape dfa_cae_forward_train refuses is refused by dfa_cae_train_plan with the same code and message (the
    messages recorded for the step in tests/golden/abi_train_errors.json)"""
    import json
    import os
    golden = {name: (code, msg) for name, code, msg in
              json.load(open(os.path.join(os.path.dirname(__file__), "golden", "abi_train_errors.json")))}
    ctx = _lib.Context.get(torch.device("cuda", 0))
    for name, args in (("precision", (2, 32, 20, 2)), ("batch_0", (0, 32, 20, _lib.PREC_BF16)), ("T_short", (2, 15, 20, _lib.PREC_BF16)),
                       ("F_24", (2, 32, 24, _lib.PREC_BF16))):
        code, msg = golden["cae_forward_train/" + name]
        assert ctx.lib.dfa_cae_train_plan(ctx.handle, *args, None, 0) == code
        assert ctx.lib.dfa_last_error(ctx.handle).decode() == msg
