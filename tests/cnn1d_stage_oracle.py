"""Float64 statements of every kernel stage of the CNN1D training step, uniform and ragged -- TEST INFRASTRUCTURE ONLY.

The model is the reference's src/model_cnn1d.py:13-46 in train mode (three Conv1d k3 + BatchNorm1d + ReLU blocks, Dropout behind
the first two, the mean over time and a Linear behind the third); a ragged batch is the definition of DESIGN.md section 3.4e
(tests/ragged_train_oracle.py).  As in tests/cae_stage_oracle.py (whose comparator, criteria and generic BatchNorm stages this
file imports, generalised there for a `valid` mask and a frame count) no stage feeds another: each takes its operands as tensors,
channel-major [B, C, T] as the product stores them, and returns what ONE kernel (or one kernel and its reduction) makes of them.
Everything the step stores is fp32; the arithmetic `dt` is a parameter (float64: the statement; float32: the CPU floor).

Read off the kernels (csrc/cnn1d_train_api.hip names the ~30 launches):
  Conv1d      conv1d_x3_kernel (conv1d_x3.hip; stored layout, 3 <= T <= 384, Cin % 4 == 0) or conv1d.hip (any strides,
              T < 3, T > 384): z = b + sum_{c,k} w[o][c][k] a[c][t + k - 1], a read as zero outside [0, lengths[b]).
  statistics  cm_stats_kernel + bn_finalize_kernel: sums over the sum-of-lengths frames of the batch, the variance biased, the
              running variance unbiased (n / (n - 1)), momentum as given.
  h1, h2      cm_bn_relu_drop_kernel: max(fma((z - mean) invstd, gamma, beta), 0) * keep-scale-or-zero, the Philox draw indexed by the
              flat [B][C][T_max] element; an exact zero at every padding frame.
  pooled      cm_bn_relu_meant_kernel: sc = gamma invstd, sh = beta - mean sc, sum_t max(fma(z, sc, sh), 0) / lengths[b].
  backward    linear_bwd_kernel (dpooled = dlogit w); cm_bn_bwd_reduce_kernel<SRC> (S1 = sum dy, S2 = sum dy xhat, dy = g where
              fma(gamma, xhat, beta) > 0; g = dpooled / lengths[b] (SRC 0) or dh * keep-scale-or-zero (SRC 1));
              cm_bn_bwd_apply_kernel (gamma invstd (dy - S1 / n - xhat S2 / n); an exact zero at every padding frame);
              conv1d_wgrad_*_kernel (dW[o][c][k] = sum dz[o][t] a[c][t + k - 1], db = sum dz; layer 1 reads x through the armed
              augmentation, time roll included); the data gradient dh = Conv1d of dz with the flipped, transposed weights.

Padding frames of a ragged batch (t >= lengths[b]).  h and dz hold exact zeros (`padding_failures`): cm_bn_relu_drop_ragged_kernel
and cm_bn_bwd_apply_ragged_kernel write them, and the uniform convolutions, weight and data gradients of layers 2 and 3 read them
as the utterance's own zero padding.  z there is written by the convolution kernels (the bias plus the taps that still reach
valid frames) and dh by the data-gradient convolutions; no stage reads either -- the statistics, h, pooled and both BatchNorm
backward kernels stop at lengths[b] -- so they only have to be finite (the region was NaN before the step): the z and dh stages
compare the valid frames (`_sel`).

Layer 3 decides ReLU with two associations (forward fma(z, gamma invstd, beta - mean gamma invstd), backward
fma(gamma, (z - mean) invstd, beta)); both are within K_BN roundings of A = |gamma| invstd (|z| + |mean|) + |beta| of the float64
value (derivation at cae_stage_oracle.bn_relu_pool), so an element whose float64 BatchNorm output lies within K_BN u A of zero is an
open decision: either branch is accepted where it is stored (dz: the other branch's distance is its allowance), it enters a sum's
bound with its own magnitude (S1, S2, pooled), and each layer's share of them is capped (AMBIGUOUS_CAP, the `l*.relu` rows).

Dropout.  The keep masks are not restated (the Philox stream is the product's own): they are READ OFF the stored h (`read_keeps`).
An element is dropped iff h is stored as an exact 0 while the float64 relu(bn(z)) exceeds its fp32 allowance K_BN u A; a kept one
must equal relu(bn(z)) / (1 - p), which the h stages check.  Where relu(bn(z)) lies within that allowance of zero the decision
cannot be read: such an element is taken as kept in h (its value is within the allowance of zero either way) and judged as an
open decision in the backward wherever its ReLU is on, which covers a dropped element (gradient 0 = the closed branch).

Convolutions under option cnn1d_train_x3 = 3 (`conv_terms=2`).  conv1d_x3_kernel<MT, 2> and pack_conv1d_terms_kernel carry each
fp32 operand v as v0 = bf16(v), v1 = bf16(v - v0) (round to nearest even: |v - v0| <= 2^-8 |v|, so |v1| <= 2^-8 (1 + 2^-8) |v|, and
|v - v0 - v1| <= 2^-16 |v|) and keep the three products w0 x0, w0 x1, w1 x0, each exact in the fp32 accumulator.  With rw, rx the
two-term residuals, w x - kept = w1 x1 + rw x + (w0 + w1) rx, at most (2^-16 (1 + 2^-8)^2 + 2^-16 + (1 + 2^-16) 2^-16) |w| |x|
<= 3.01 * 2^-16 |w| |x|.  The fp32 floor does not apply there: the element's allowance is C_X2 2^-16 sum |a| |w| + K u A with
C_X2 = 3.01, K = 3 Cin + 1 the fp32 additions of the products and the bias, A = sum |a| |w| + |b|.  The default (three terms, six
products) drops only pairs below 2^-24 of a product and is held to the fp32 criterion.
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

from cae_stage_oracle import (AMBIGUOUS_CAP, BN_EPS, F32, F64, K_BN, U, Result, Row, Stage, batch_stats, bn_bwd_apply,  # noqa: F401
                              bn_bwd_reduce, bn_relu_pool, compare, compare_one, f32r, invstd_of, print_rows, row_failures)

BN_C = (32, 64, 128)
CONV, BNL = ("conv.0", "conv.4", "conv.8"), ("conv.1", "conv.5", "conv.9")
PARAM_ORDER = [f"{p}.{k}" for c, b in zip(CONV, BNL) for p in (c, b) for k in ("weight", "bias")] + ["classifier.weight", "classifier.bias"]
MOMENTUM, SMOOTHING = 0.1, 0.05
C_X2 = 3.01          # two-term convolutions: the dropped products, in units of 2^-16 |w| |x| (module docstring)

# The uniform cases of tests/test_cnn1d_train_stages_gpu.py (B, T, F): below the matrix-core kernel's T >= 3; its minimum; the
# 32-frame tile and an F whose k-steps are padded to an even count; the 64-frame weight-gradient slab; F % 4 != 0 (layer 1 on the
# strided kernel); the 256-thread stride of the reductions; the real shape; the two sides of the T <= 384 switch; a reduction chunk
# with two utterances and empty trailing chunks; empty weight-gradient chunks
CASES = [(3, 2, 20), (1, 3, 20), (2, 33, 36), (3, 65, 20), (2, 31, 31), (2, 257, 20), (2, 321, 180), (1, 384, 20), (1, 385, 20),
         (70, 5, 20), (257, 3, 20)]
# The ragged sets of tests/test_cnn1d_ragged_train_gpu.py: name -> (lengths, T_max, F)
RAGGED = {
    "A": ([37, 3, 20, 36, 5], 40, 20),
    "B": ([321, 64, 257], 324, 180),
    "C": ([130, 400], 400, 20),
    "D": ([int(v) for v in np.random.default_rng(70).integers(3, 49, 70)], 48, 20),
}


def ordinary_state(seed, F_):
    """state_dict of a default-initialised CNN1D with gamma uniform in [0.5, 1.5], beta = 0.1 randn and a classifier scaled so
    that logits are of order 1 (the recipe of tests/ragged_train_oracle.py::cnn1d_state)"""
    from dfa_amd.model_cnn1d import CNN1D
    torch.manual_seed(seed)
    m = CNN1D(in_features=F_, dropout=0.0)
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for i in m._BN_IDX:
            m.conv[i].weight.copy_(0.5 + torch.rand(m.conv[i].weight.shape, generator=g))
            m.conv[i].bias.copy_(0.1 * torch.randn(m.conv[i].bias.shape, generator=g))
        m.classifier.weight.mul_(40.0)
    return {k: v.detach().clone() for k, v in m.state_dict().items()}


def case_input(B, T, F_, lengths=None, seed=None, pad=float("nan")):
    """(stored [B, F, T] = 3.2 randn - 0.07 (the LFCC-like scale of the training tests), every frame t >= lengths[b] set to `pad`;
    y [B] random 0/1), float32"""
    g = torch.Generator().manual_seed(3000 + B + T + F_ if seed is None else seed)
    x = torch.randn(B, F_, T, generator=g) * 3.2 - 0.07
    y = (torch.rand(B, generator=g) > 0.5).float()
    for b, t in enumerate(lengths or ()):
        x[b, :, int(t):] = pad
    return x, y


def keep_scale(p):
    """1 / (1 - p) as train_host.h::drop_cfg forms it in float32"""
    return float(np.float32(1.0) / (np.float32(1.0) - np.float32(p)))


def valid_mask(lengths, B, T):
    """bool [B, 1, T]: frame t belongs to utterance b (all True for a uniform batch)"""
    if lengths is None:
        return torch.ones(B, 1, T, dtype=torch.bool)
    return (torch.arange(T)[None, :] < torch.tensor([int(v) for v in lengths])[:, None]).unsqueeze(1)


def _cl(t):
    """[B, C, T] -> the [B, T, 1, C] the generic BatchNorm stages take (a valid mask [B, 1, T] -> [B, T, 1, 1])"""
    return t.permute(0, 2, 1).unsqueeze(2)


def _cm(t):
    return t.squeeze(2).permute(0, 2, 1)


def _zeroed(t, valid):
    """t with everything outside the utterances read as zero, as the kernels' loads read it (padding may hold NaN)"""
    return torch.where(valid, t, torch.zeros_like(t))


# ------------------------------------------------------------------------------------------------------------------- stages
def conv1d(a, w, b, valid, dt=F64, mags=False):
    """a [B,Cin,T], w [Cout,Cin,3], b [Cout] -> the pre-BatchNorm output [B,Cout,T]: zero padding 1 at each utterance's own two
    ends.  K = 3 Cin + 1 terms summed in fp32."""
    a_, w_, b_ = _zeroed(a.to(dt), valid), w.to(dt), b.to(dt)
    out = F.conv1d(a_, w_, b_, padding=1)
    A = F.conv1d(a_.abs(), w_.abs(), b_.abs(), padding=1) if mags else None
    return Stage(out, A, 3 * w.shape[1] + 1)


def conv1d_dgrad(dz, w, valid, dt=F64, mags=False):
    """dz [B,Cout,T] (zero at padding), w [Cout,Cin,3] -> the gradient of the layer's input [B,Cin,T]: tap k of the forward reaches
    frame t from dz[t - k + 1], i.e. a Conv1d with the taps FLIPPED and the channels transposed.  K = 3 Cout terms."""
    dz_, w_ = _zeroed(dz.to(dt), valid), w.to(dt)
    out = F.conv_transpose1d(dz_, w_, padding=1)
    A = F.conv_transpose1d(dz_.abs(), w_.abs(), padding=1) if mags else None
    return Stage(out, A, 3 * w.shape[0])


def conv1d_wgrad(dz, a, valid, dt=F64):
    """dz [B,Cout,T], the layer's input a [B,Cin,T] -> (dW [Cout,Cin,3], db [Cout]): dW[o][c][k] = sum_{b,t} dz[b][o][t] a[b][c][t+k-1]
    over each utterance's own frames"""
    dz_, a_ = _zeroed(dz.to(dt), valid), F.pad(_zeroed(a.to(dt), valid), (1, 1))
    T = dz.shape[2]
    dW = torch.stack([torch.einsum("bot,bct->oc", dz_, a_[:, :, k:k + T]) for k in range(3)], dim=2)
    return dW, dz_.sum(dim=(0, 2))


def bn_relu_drop(z, mean, invstd, gamma, beta, valid, keep=1.0, sc=1.0, dt=F64, mags=False):
    """h = relu(bn(z)) * keep * sc at an utterance's own frames, zero at padding; K = K_BN (+ 1 for the keep-scale product)"""
    st = bn_relu_pool(_cl(_zeroed(z, valid)), mean, invstd, gamma, beta, 1, dt, mags)
    f = (valid.to(dt) * keep * sc) if isinstance(keep, torch.Tensor) else valid.to(dt) * (keep * sc)
    return Stage(_cm(st.out) * f, None if st.A is None else _cm(st.A) * f.abs(), st.K + 1)


def time_mean(z, mean, invstd, gamma, beta, lengths_t, valid, dt=F64, mags=False):
    """z [B,128,T] -> (pooled [B,128] = the mean over the utterance's own lengths[b] frames of relu(fma(z, sc, sh)), slack: what
    the open ReLU decisions can move it by)"""
    z_, mean_, invstd_, gamma_, beta_ = (t.to(dt) for t in (_zeroed(z, valid), mean, invstd, gamma, beta))
    s = (gamma_ * invstd_)[None, :, None]
    r = F.relu(z_ * s + (beta_ - mean_ * gamma_ * invstd_)[None, :, None])
    out = _zeroed(r, valid).sum(dim=2) / lengths_t.to(dt)[:, None]
    slack = None
    if mags:       # the open decisions only (decided in float64 whatever dt is, as bn_bwd_reduce's amb), each with its own magnitude
        z64, m64, i64, g64, b64 = (t.to(F64) for t in (_zeroed(z, valid), mean, invstd, gamma, beta))
        s64 = (g64 * i64)[None, :, None]
        y = z64 * s64 + (b64 - m64 * g64 * i64)[None, :, None]
        terms = s64.abs() * (z64.abs() + m64.abs()[None, :, None]) + b64.abs()[None, :, None]
        amb = (y.abs() <= K_BN * U * terms) & valid
        slack = (K_BN * U * terms * amb).sum(dim=2) / lengths_t.to(F64)[:, None]
    return out, slack


def bce_smooth(logits, y, eps=SMOOTHING, dt=F64):
    """BCEWithLogitsLoss(mean) on y (1 - eps) + eps / 2 -> (loss, dlogits [B])"""
    z, ys = logits.to(dt), y.to(dt) * (1.0 - eps) + 0.5 * eps
    return F.binary_cross_entropy_with_logits(z, ys), (torch.sigmoid(z) - ys) / z.numel()


def classifier_backward(dlogits, pooled, w, dt=F64):
    """dlogits [B], pooled [B,128], w [1,128] -> (dpooled [B,128], dW [1,128], db [1])"""
    d, e, w_ = dlogits.to(dt), pooled.to(dt), w.to(dt)
    return d[:, None] * w_.reshape(1, -1), (d[:, None] * e).sum(dim=0, keepdim=True), d.sum().reshape(1)


def upstream(o, l, valid, dt=F64):
    """the gradient that arrives at layer l's BatchNorm + ReLU output [B,C,T]: dpooled / lengths[b] at every own frame (layer 3), or
    dh * keep * keep-scale (layers 1 and 2); zero at padding"""
    if l == 2:
        B, _, T = o["z"][2].shape
        up = (o["dpooled"].to(dt) / o["lengths_t"].to(dt)[:, None])[:, :, None].expand(-1, -1, T)
    else:
        k = o["keep"][l]
        up = o["dh"][l].to(dt) * ((k.to(dt) if isinstance(k, torch.Tensor) else k) * (keep_scale(o["p"]) if o["p"] > 0 else 1.0))
    return _zeroed(up, valid)


# ------------------------------------------------------------------------------------------------------------------ the chain
def _params(sd, dt=F64):
    return {k: (v if isinstance(v, torch.Tensor) else torch.from_numpy(np.asarray(v))).detach().cpu().to(dt) for k, v in sd.items()
            if not k.endswith("num_batches_tracked")}


def _bnp(o, P, l):
    return o["mean"][l], o["invstd"][l], P[BNL[l] + ".weight"], P[BNL[l] + ".bias"]


def new_operands(x, y, lengths, p=0.0, keeps=None):
    """the frame of an operand set: x [B,F,T] channel-major (as the layer-1 kernels see it, augmentation included), labels,
    lengths (None: uniform), the frame count n BatchNorm runs over"""
    B, _, T = x.shape
    lt = torch.tensor([T] * B if lengths is None else [int(v) for v in lengths], dtype=F64)
    k = [1.0, 1.0] if keeps is None else [t.to(F64) for t in keeps]
    return {"x": x.detach().cpu().to(F64), "y": y.detach().cpu().to(F64), "lengths": None if lengths is None else [int(v) for v in lengths],
            "lengths_t": lt, "n": int(lt.sum()), "p": p, "keep": k, "valid": valid_mask(lengths, B, T), "z": [None] * 3, "h": [None] * 2,
            "dz": [None] * 3, "dh": [None] * 2, "mean": [None] * 3, "var": [None] * 3, "invstd": [None] * 3, "run": [None] * 3, "grads": {}}


def run_chain(sd, x, y, lengths=None, fp32_points=True, p=0.0, keeps=None, momentum=MOMENTUM):
    """One training step as a chain of the stages in float64 -> the operand set `stage_results` reads.  fp32_points: every tensor
    the product stores is rounded to fp32 where it is stored (the operands of the CPU tests); False: no rounding anywhere (must
    equal the autograd oracles).  p, keeps = (keep1 [B,32,T], keep2 [B,64,T]): dropout with given masks."""
    P = _params(sd)
    r = f32r if fp32_points else (lambda t: t)
    o = new_operands(x, y, lengths, p, keeps)
    o["x"] = _zeroed(o["x"], o["valid"])
    v, g, n = o["valid"], o["grads"], o["n"]
    sc = keep_scale(p) if p > 0 else 1.0
    a = o["x"]
    for l in range(3):
        o["z"][l] = r(conv1d(a, P[CONV[l] + ".weight"], P[CONV[l] + ".bias"], v).out)
        m, var = batch_stats(_cl(o["z"][l]), F64, _cl(v))
        o["mean"][l], o["var"][l], o["invstd"][l] = r(m), r(var), r(invstd_of(r(var)))
        rm, rv = P[BNL[l] + ".running_mean"], P[BNL[l] + ".running_var"]
        o["run"][l] = (r((1 - momentum) * rm + momentum * m), r((1 - momentum) * rv + momentum * var * (n / max(n - 1, 1))))
        if l < 2:
            a = o["h"][l] = r(bn_relu_drop(o["z"][l], *_bnp(o, P, l), v, o["keep"][l], sc).out)
    o["pooled"] = r(time_mean(o["z"][2], *_bnp(o, P, 2), o["lengths_t"], v)[0])
    o["logits"] = r(F.linear(o["pooled"], P["classifier.weight"], P["classifier.bias"]).squeeze(-1))
    loss, dl = bce_smooth(o["logits"], o["y"])
    o["loss"], o["dlogits"] = float(loss), r(dl)
    dp, g["classifier.weight"], g["classifier.bias"] = classifier_backward(o["dlogits"], o["pooled"], P["classifier.weight"])
    o["dpooled"] = r(dp)
    for l in (2, 1, 0):
        stt = _bnp(o, P, l)
        up = upstream(o, l, v)
        red = bn_bwd_reduce(_cl(o["z"][l]), _cl(up), *stt, valid=_cl(v))
        g[BNL[l] + ".bias"], g[BNL[l] + ".weight"] = r(red.S1), r(red.S2)
        dz = bn_bwd_apply(_cl(o["z"][l]), _cl(up), *stt, g[BNL[l] + ".bias"], g[BNL[l] + ".weight"], n=n)[0].out
        o["dz"][l] = r(_zeroed(_cm(dz), v))
        g[CONV[l] + ".weight"], g[CONV[l] + ".bias"] = conv1d_wgrad(o["dz"][l], o["x"] if l == 0 else o["h"][l - 1], v)
        if l > 0:
            o["dh"][l - 1] = r(conv1d_dgrad(o["dz"][l], P[CONV[l] + ".weight"], v).out)
    o["sums"] = [torch.stack([g[b + ".bias"], g[b + ".weight"]], dim=1) for b in BNL]
    return o


# -------------------------------------------------------------------------------------- every stage on one set of stored tensors
def read_keeps(o, sd):
    """The dropout keep masks of a step, read off its stored h1 and h2 (module docstring) -> ((keep1, keep2) bool [B,C,T], (determined1,
    determined2) bool: the own-frame elements whose undropped value exceeds its fp32 allowance)"""
    P = _params(sd)
    keeps, det = [], []
    for l in (0, 1):
        st = bn_relu_drop(o["z"][l], *_bnp(o, P, l), o["valid"], 1.0, 1.0, F64, True)
        d = (st.out > st.K * U * st.A) & o["valid"]
        keeps.append(~((o["h"][l] == 0) & d))
        det.append(d)
    return tuple(keeps), tuple(det)


def padding_failures(o):
    """h and dz are exact zeros at every padding frame of a ragged batch"""
    pad = ~o["valid"]
    bad = []
    for name, ts in (("h", o["h"]), ("dz", o["dz"])):
        for l, t in enumerate(ts):
            if not bool((t[pad.expand(t.shape)] == 0).all()):
                bad.append(f"{name}{l + 1} is not an exact zero at every padding frame")
    return bad


def stage_results(o, sd, dt=F64, mags=True, conv_terms=3, momentum=MOMENTUM):
    """Every stage evaluated in `dt` on the stored tensors `o` (the layout of run_chain's result; o["grads"] gives the sums the apply
    passes read, o["keep"] the dropout masks (1.0: none), o["det"] (optional) read_keeps' determined elements) -> {stage name:
    Result}.  mags=False (the float32 floor run): values only.  conv_terms=2: the run's five convolutions used two bf16 terms per
    operand (module docstring)."""
    P = _params(sd)
    R = {}
    v, G, n, p = o["valid"], o["grads"], o["n"], o["p"]
    vb = {c: v.expand(-1, c, -1) for c in BN_C + (o["x"].shape[1],)}
    sc = keep_scale(p) if p > 0 else 1.0
    det = o.get("det", (None, None))
    x2 = mags and conv_terms == 2

    def _sel(t, c):
        """the own frames of a [B,c,T] tensor (what z and dh hold at padding is read by no stage)"""
        return t if o["lengths"] is None or t is None else t[vb[c]]

    def conv_result(st, c):
        if not x2:
            return Result("fp32", _sel(st.out, c))
        return Result("allow", _sel(st.out, c), slack=_sel((C_X2 * 2.0 ** -16 + st.K * U) * st.A, c))    # the allowance alone: no floor

    for l in range(3):
        a = o["x"] if l == 0 else o["h"][l - 1]
        w, b = P[CONV[l] + ".weight"], P[CONV[l] + ".bias"]
        name = f"l{l + 1}"
        R[name + ".z"] = conv_result(conv1d(a, w, b, v, dt, x2), BN_C[l])
        m, var = batch_stats(_cl(o["z"][l]), dt, _cl(v))
        R[name + ".mean"], R[name + ".var"] = Result("fp32", m), Result("fp32", var)
        R[name + ".invstd"] = Result("fp32", invstd_of(o["var"][l].to(dt)))             # (against the stored variance)
        rm, rv = P[BNL[l] + ".running_mean"].to(dt), P[BNL[l] + ".running_var"].to(dt)        # sd: the state before the step
        R[name + ".running_mean"] = Result("fp32", (1 - momentum) * rm + momentum * m)
        R[name + ".running_var"] = Result("fp32", (1 - momentum) * rv + momentum * var * (n / max(n - 1, 1)))
        if l < 2:
            R[name + ".h"] = Result("fp32", bn_relu_drop(o["z"][l], *_bnp(o, P, l), v, o["keep"][l], sc, dt).out)
    pooled, sl = time_mean(o["z"][2], *_bnp(o, P, 2), o["lengths_t"], v, dt, mags)
    R["pooled"] = Result("fp32", pooled, slack=sl)
    R["logits"] = Result("fp32", F.linear(o["pooled"].to(dt), P["classifier.weight"].to(dt), P["classifier.bias"].to(dt)).squeeze(-1))
    loss, dl = bce_smooth(o["logits"], o["y"], SMOOTHING, dt)
    R["bce.loss"], R["bce.dlogits"] = Result("fp32", loss.reshape(1)), Result("fp32", dl)
    # ---- backward
    dp, dWc, dbc = classifier_backward(o["dlogits"], o["pooled"], P["classifier.weight"], dt)
    R["cls.dpooled"], R["classifier.weight"], R["classifier.bias"] = Result("fp32", dp), Result("fp32", dWc), Result("fp32", dbc)
    for l in (2, 1, 0):
        name, stt = f"l{l + 1}", _bnp(o, P, l)
        up = upstream(o, l, v, dt)
        also = None if l == 2 or det[l] is None else _cl(~det[l])
        red = bn_bwd_reduce(_cl(_zeroed(o["z"][l], v)), _cl(up), *stt, dt, also_open=also, valid=_cl(v))
        R[BNL[l] + ".weight"] = Result("fp32", red.S2, slack=red.slack2 if mags else None)
        R[BNL[l] + ".bias"] = Result("fp32", red.S1, slack=red.slack1 if mags else None)
        ap, alt = bn_bwd_apply(_cl(_zeroed(o["z"][l], v)), _cl(up), *stt, G[BNL[l] + ".bias"], G[BNL[l] + ".weight"], dt, n=n)
        want = _zeroed(_cm(ap.out), v)
        slack = None
        if mags:
            slack = torch.where(_cm(red.amb), (_cm(alt).to(F64) - want.to(F64)).abs(), torch.zeros_like(want, dtype=F64))
            R[name + ".relu"] = Result("share", torch.tensor(float(red.amb.double().sum()) / (n * BN_C[l])))
        R[name + ".dz"] = Result("fp32", want, slack=slack)
        dW, db = conv1d_wgrad(o["dz"][l], o["x"] if l == 0 else o["h"][l - 1], v, dt)
        R[CONV[l] + ".weight"] = Result("fp32", dW)
        # (a sum that cancels to rounding residue: measured against the largest channel sum of |dz|)
        R[CONV[l] + ".bias"] = Result("fp32", db, scale=max(float(_zeroed(o["dz"][l], v).abs().sum(dim=(0, 2)).max()), 1e-300))
        if l > 0:
            R[name + ".dx"] = conv_result(conv1d_dgrad(o["dz"][l], P[CONV[l] + ".weight"], v, dt, x2), BN_C[l - 1])
    return R


STORED = {"pooled": "pooled", "logits": "logits", "bce.dlogits": "dlogits", "cls.dpooled": "dpooled"}


def stored_of(o, name):
    """the stored counterpart of stage `name` in an operand set (z and dh: their own frames only)"""
    if name in o["grads"]:
        return o["grads"][name]
    if name in STORED:
        return o[STORED[name]]
    if name == "bce.loss":
        return torch.tensor([o["loss"]], dtype=F64)
    head, _, tail = name.partition(".")
    l = int(head[1]) - 1
    if tail in ("mean", "var", "invstd"):
        return o[tail][l]
    if tail in ("running_mean", "running_var"):
        return o["run"][l][tail == "running_var"]
    if tail in ("h", "dz"):
        return o[tail][l]
    t = o["z"][l] if tail == "z" else o["dh"][l - 1]
    return t if o["lengths"] is None else t[o["valid"].expand(t.shape)]


def stage_names():
    """every stage that compares a stored tensor"""
    names = set(PARAM_ORDER) | set(STORED) | {"bce.loss", "l1.h", "l2.h", "l2.dx", "l3.dx"}
    return names | {f"l{l}.{k}" for l in (1, 2, 3) for k in ("z", "dz", "mean", "var", "invstd", "running_mean", "running_var")}


def kept_share_failures(keeps, det, p):
    """the kept share of the determined elements lies within 5 sigma + 2^-16 of 1 - p (csrc/rng.h compares 16-bit uniforms with the
    top 16 bits of p 2^32: the rate is p to within 2^-16)"""
    bad = []
    for l, (k, d) in enumerate(zip(keeps, det)):
        cnt = int(d.sum())
        share = float(k[d].double().mean())
        if not abs(share - (1 - p)) < 5 * math.sqrt(p * (1 - p) / cnt) + 2.0 ** -16:
            bad.append(f"layer {l + 1}: kept share {share:.4f} of {cnt} determined elements, p = {p}")
    return bad
