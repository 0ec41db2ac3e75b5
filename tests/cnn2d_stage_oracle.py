"""Float64 statements of every kernel stage of the CNN2D training step -- TEST INFRASTRUCTURE ONLY.

The model is the reference's src/model.py:13-39 in train mode (three Conv2d 3x3 + BatchNorm + ReLU blocks, AvgPool2d((2, 1)) and
Dropout behind the first two, the mean over time and a Linear behind the third); the rounding points are the ones
oracle/torch_ref.py::cnn2d_train_step_emulated documents.  As in tests/cae_stage_oracle.py (whose comparator, criteria and
generic stages this file imports) no stage feeds another: each takes its operands as tensors, channels-last as the product
stores them ([B, H, F, C]; weights in torch's layouts), and returns what ONE kernel (or one kernel and its reduction) makes of
them.  The arithmetic `dt` is a parameter (float64: the statement; float32: the CPU floor); with mags=True a stage also returns
A (the sum of the magnitudes of an element's terms) and K (the fp32 roundings spent on them).

Rounding points, read off the kernels (csrc/train_api.hip names the launches):
  block 1     conv1.hip / train_conv1.hip / train_conv1_mfma.hip: fp32 weights folded with the batch statistics (fw = w s,
              fb = (b - mean) s + beta), nine products and the bias in fp32, ReLU, the pair average, the dropout keep-scale, ONE
              rounding to the storage type.  z1 is never stored; its statistics are fp32 sums of the unrounded z1 over ALL T rows.
  conv 2, 3   conv_split.hip / conv3_m16.hip: stored activation times bf16(w) (bf16 mode; the fp32 mode's three-term split
              carries w to 2^-18 of a product) + bias in fp32, one rounding to the storage type; the statistics are the
              epilogue's fp32 sums of the UNROUNDED accumulators.
  a2          train_elem.hip::bn_relu_poolh2_drop_kernel: sc = gamma invstd, sh = beta - mean sc, 0.5 (relu(fma(z0, sc, sh)) +
              relu(fma(z1, sc, sh))) ds, one rounding.
  emb, msum   bn_relu_meant_kernel: acc += relu(fma(z, sc, sh)) in t order, emb = acc / H; n += mask, sx += mask xhat with
              xhat = (z - mean) invstd, mask = fma(gamma, xhat, beta) > 0 -- the backward kernels' formulas.
  backward    linear_bwd_kernel (demb = dlogit w, transposed to [B][F][128]); bn_bwd_reduce_saved_kernel (S1 = sum g n,
              S2 = sum g sx, g = demb / H); bn_bwd_apply_meant_kernel / bn_bwd_apply_pool_kernel / bn_bwd_apply_kernel<SRC_POOL>
              (k0 (dy - k1 - xhat k2), one rounding); the weight gradients multiply two stored tensors, the data gradients a
              stored tensor and bf16(w); block 1 recomputes z1 from x.

Dropout.  The keep masks are not restated (the Philox stream is the product's own): they are READ OFF the stored tensors.  An
element of a1 / a2 is dropped iff it is stored as 0 while its float64 undropped value exceeds its own allowance
(2^-8 |want| + K u A); kept elements must equal want / (1 - p).  An element whose undropped value lies within its allowance of
zero is undetermined -- and cannot matter: the pooled value is half the sum of two ReLU outputs, both >= 0, so both lie within
that allowance of zero: each ReLU is closed, or its input is positive and that small.  In the backward such an element's
upstream gradient is multiplied by those two masks: zero where the ReLU is closed; where it is not, the element is judged as an
open decision (`open_rows`, or-ed into `bn_bwd_reduce`'s amb: both branches are accepted and its magnitude enters the sums'
bounds), which covers a dropped element (gradient 0 = the closed branch) as well as a kept one.  It is taken as kept.
Where the mask of layer 1 is applied differs by path: with the matrix-core block 1 (train_c1_mfma) the 16x16x32 data-gradient
kernel applies it where da1 is produced (csrc/train_api.hip: `a.drop = dc` before launch_dgrad2) and the stored da1 is exactly 0
at every dropped position; otherwise da1 is stored unmasked and the block-1 backward applies it (train_conv1.hip, drop_scale8).
`da1_masked` says which statement holds; undetermined elements may be stored either way.

`run_chain` strings the stages together (float64, roundings on or off), `stage_results` evaluates every stage on one set of
stored tensors, `CASES` / `ordinary_state` / `case_input` are what tests/test_cnn2d_train_stages_{cpu,gpu}.py run.
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

from cae_stage_oracle import (AMBIGUOUS_CAP, BN_EPS, F32, F64, HALF_BF16, K_BLOCK1, K_BN, U, UNEQUAL_CAP, Result, Row, Stage,  # noqa: F401
                              batch_stats, bf16, block1_backward, block1_forward, bn_bwd_apply, bn_bwd_reduce, bn_relu_pool, compare,
                              compare_one, conv3x3, conv3x3_dgrad, conv3x3_wgrad, f32r, invstd_of, print_rows, row_failures,
                              unequal_share, upstream)

BN_C = (32, 64, 128)
CONV, BNL = ("conv.0", "conv.5", "conv.10"), ("conv.1", "conv.6", "conv.11")
PARAM_ORDER = [f"{p}.{k}" for c, b in zip(CONV, BNL) for p in (c, b) for k in ("weight", "bias")] + ["classifier.weight", "classifier.bias"]
MOMENTUM, SMOOTHING = 0.1, 0.05

# The cases of tests/test_cnn2d_train_stages_gpu.py: the smallest T the ABI takes (H2 = 1); odd at both pool levels (7 -> 3 -> 1:
# a dropped row under a live mask in blocks 1 and 2), F one short of a 32-column strip and one over a 30-column strip; one column
# into the second strip of both widths; the two ragged shapes of tests/test_train_shapes_gpu.py; the real shape (frame 320
# dropped, six 30-column strips); H1 = 161, a dropped row at both levels
CASES = [(1, 4, 5), (2, 7, 31), (2, 10, 33), (3, 21, 65), (2, 33, 5), (2, 321, 180), (2, 323, 180)]


def ordinary_state(seed, F_):
    """state_dict of a default-initialised CNN2D with gamma uniform in [0.5, 1.5], beta = 0.1 randn and a classifier scaled so
    that logits are of order 1 (the recipe of tests/test_train_shapes_gpu.py::_random_cnn2d_state)"""
    from dfa_amd.model import CNN2D
    torch.manual_seed(seed)
    m = CNN2D(in_features=F_, dropout=0.0)
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for i in (1, 6, 11):
            m.conv[i].weight.copy_(0.5 + torch.rand(m.conv[i].weight.shape, generator=g))
            m.conv[i].bias.copy_(0.1 * torch.randn(m.conv[i].bias.shape, generator=g))
        m.classifier.weight.mul_(40.0 * math.sqrt(180.0 / F_))
    return {k: v.detach().clone() for k, v in m.state_dict().items()}


def case_input(B, T, F_, seed=None):
    """(x [B,T,F] = 3.2 randn - 0.07 rounded to bf16 (the LFCC-like scale of the training tests), y [B] random 0/1), float32"""
    g = torch.Generator().manual_seed(2000 + B + T + F_ if seed is None else seed)
    x = (torch.randn(B, T, F_, generator=g) * 3.2 - 0.07).to(torch.bfloat16).float()
    return x, (torch.rand(B, generator=g) > 0.5).float()


def keep_scale(p):
    """1 / (1 - p) as train_host.h::drop_cfg forms it in float32"""
    return float(np.float32(1.0) / (np.float32(1.0) - np.float32(p)))


# ------------------------------------------------------------------------------------------------------------------- stages
def tap_moments(x, dt=F64):
    """x [B,T,F] -> (XX [9,9] = sum over pixels of x_j x_k, Xs [9] = sum of x_k), x_k the k-th tap of the zero-padded 3x3 window:
    what the statistics pass leaves for the one-pass block-1 backward (train_conv1.hip, STATS_XX)"""
    B, T, Fq = x.shape
    xp = F.pad(x.to(dt), (1, 1, 1, 1))
    taps = torch.stack([xp[:, ky:ky + T, kx:kx + Fq] for ky in range(3) for kx in range(3)], dim=-1).reshape(-1, 9)
    return taps.T @ taps, taps.sum(dim=0)


def time_mean(z3, mean, invstd, gamma, beta, dt=F64):
    """z3 [B,H,F,128] as stored -> (emb [B,128,F] = mean_t ReLU(BatchNorm(z3)), n [B,F,128] = sum_t mask, sx = sum_t mask xhat,
    slack_n, slack_sx: what the open ReLU decisions (cae_stage_oracle.bn_bwd_reduce's amb) can move the two sums by).  The mask
    and its count are decisions, not arithmetic: they are taken in float64 whatever dt is."""
    z, mean_, invstd_, gamma_, beta_ = (t.to(dt) for t in (z3, mean, invstd, gamma, beta))
    s = gamma_ * invstd_
    emb = F.relu(z * s + (beta_ - mean_ * s)).mean(dim=1).permute(0, 2, 1).contiguous()
    z64, m64, i64, g64, b64 = (t.to(F64) for t in (z3, mean, invstd, gamma, beta))
    xh64 = (z64 - m64) * i64
    y64 = g64 * xh64 + b64
    on = y64 > 0
    amb = y64.abs() <= K_BN * U * (g64.abs() * i64 * (z64.abs() + m64.abs()) + b64.abs())
    xh = (z - mean_) * invstd_
    n = on.to(dt).sum(dim=1)
    sx = torch.where(on, xh, torch.zeros_like(xh)).sum(dim=1)
    return emb, n, sx, amb.to(F64).sum(dim=1), (amb * xh64.abs()).sum(dim=1)


def bce_smooth(logits, y, eps=SMOOTHING, dt=F64):
    """BCEWithLogitsLoss(mean) on y (1 - eps) + eps / 2 -> (loss, dlogits [B])"""
    z, ys = logits.to(dt), y.to(dt) * (1.0 - eps) + 0.5 * eps
    return F.binary_cross_entropy_with_logits(z, ys), (torch.sigmoid(z) - ys) / z.numel()


def classifier_backward(dlogits, emb, w, dt=F64):
    """dlogits [B], emb [B,128,F], w [1,128 F] -> (demb [B,F,128] (transposed for the BatchNorm backward), dW [1,128 F], db [1])"""
    d, e, w_ = dlogits.to(dt), emb.to(dt), w.to(dt)
    B, C, Fq = emb.shape
    demb = (d[:, None] * w_.reshape(1, -1)).reshape(B, C, Fq).permute(0, 2, 1).contiguous()
    return demb, (d[:, None] * e.reshape(B, -1)).sum(dim=0, keepdim=True), d.sum().reshape(1)


def saved_sums(demb, n, sx, H, dt=F64):
    """block 3's BatchNorm reduction from the forward's saved sums: S1 = sum_{b,f} g n, S2 = sum_{b,f} g sx, g = demb / H"""
    g = demb.to(dt) / H
    return (g * n.to(dt)).sum(dim=(0, 1)), (g * sx.to(dt)).sum(dim=(0, 1))


def open_rows(det, H):
    """read_keeps' undetermined pooled elements [B,H/2,F,C] as a mask over the rows they were pooled from [B,H,F,C] (a dropped
    last row belongs to no pooled element); None without dropout"""
    if det is None:
        return None
    und = (~det).repeat_interleave(2, dim=1)
    return F.pad(und, (0, 0, 0, 0, 0, H - und.shape[1]))


def block1_record(x, w, b, gamma, beta, mean, invstd, da1s, dt=F64, slack=False, also_open=None):
    """the one-pass block-1 backward's [32][11] record before its algebra: A[c][k] = sum dy x_k, S1 = sum dy, S2 = sum dy xhat with
    dy = mask * 0.5 * da1s un-pooled (da1s: the stored da1 times keep mask and keep-scale) -> (A [32,9], S1, S2, slacks or None)"""
    B, T, Fq = x.shape
    x4 = x.unsqueeze(-1)
    zs = conv3x3(x4, w, b, dt, mags=slack)
    up = upstream(da1s, T, Fq, "pool21", dt)
    terms = ((gamma * invstd).abs() * (zs.A + mean.abs()) + beta.abs()) if slack else None
    red = bn_bwd_reduce(zs.out, up, mean, invstd, gamma, beta, dt, K_BLOCK1, terms, also_open)
    A = conv3x3_wgrad(torch.where(red.on, up, torch.zeros_like(up)), x4, dt)[0].reshape(32, 9)
    sl = None
    if slack:
        sl = (conv3x3_wgrad(up.abs() * red.amb, x4.abs(), F64)[0].reshape(32, 9), red.slack1, red.slack2)
    return A, red.S1, red.S2, sl


# ------------------------------------------------------------------------------------------------------------------ the chain
def _params(sd, dt=F64):
    return {k: (v if isinstance(v, torch.Tensor) else torch.from_numpy(np.asarray(v))).detach().cpu().to(dt) for k, v in sd.items()
            if not k.endswith("num_batches_tracked")}


def _bnp(o, P, l):
    return o["mean"][l], o["invstd"][l], P[BNL[l] + ".weight"], P[BNL[l] + ".bias"]


def run_chain(sd, x, y, rounding=True, fp32_points=None, autograd_xhat=False, p=0.0, keeps=None):
    """One training step as a chain of the stages in float64.  rounding=False: no rounding anywhere (must equal
    cnn2d_train_step_emulated(emulate=None)).  rounding=True: every tensor the product stores in bf16 is rounded where it is
    stored and the matrix-core convolutions take bf16 weights; fp32_points (default: as rounding) also rounds to fp32 what the
    product keeps in fp32 (statistics, sums, emb, msum, demb, logits, dlogits) -- the operands of the CPU tests.
    autograd_xhat: the S2 term of blocks 2 and 3's dz takes xhat from the UNROUNDED accumulators, which is what torch autograd
    makes of cnn2d_train_step_emulated's statistics-of-the-accumulators (the kernels take the stored z for both: the one place
    where that oracle and the product differ by more than summation order).  p, keeps = (keep1 [B,H1,F,32], keep2 [B,H2,F,64]):
    dropout with given masks.  -> the operand set `stage_results` reads."""
    P = _params(sd)
    r = bf16 if rounding else (lambda t: t)
    r32 = f32r if (rounding if fp32_points is None else fp32_points) else (lambda t: t)
    x = r(x.detach().cpu().to(F64))
    B, T, Fq = x.shape
    sc = keep_scale(p) if p > 0 else 1.0
    k1, k2 = (t.to(F64) for t in keeps) if keeps is not None else (1.0, 1.0)
    o = {"x": x, "y": y.detach().cpu().to(F64), "p": p, "mean": [None] * 3, "var": [None] * 3, "invstd": [None] * 3, "n": [0] * 3,
         "grads": {}, "keep": [k1, k2], "run0": [(P[b + ".running_mean"], P[b + ".running_var"]) for b in BNL]}
    g = o["grads"]

    def keep_stats(l, zsrc):
        m, v = batch_stats(zsrc)
        o["mean"][l], o["var"][l], o["invstd"][l], o["n"][l] = r32(m), r32(v), r32(invstd_of(v)), zsrc.numel() // zsrc.shape[-1]
    w1, b1 = P["conv.0.weight"], P["conv.0.bias"]
    keep_stats(0, conv3x3(x.unsqueeze(-1), w1, b1).out)
    o["XX"], o["Xs"] = (r32(t) for t in tap_moments(x))
    mean, istd, gam, bet = _bnp(o, P, 0)
    o["a1"] = r(block1_forward(x, w1, b1, gam, bet, mean, istd, pool=(2, 1)).out * k1 * sc)
    zu2 = conv3x3(o["a1"], r(P["conv.5.weight"]), P["conv.5.bias"]).out
    o["z2"] = r(zu2)
    keep_stats(1, zu2)
    o["a2"] = r(bn_relu_pool(o["z2"], *_bnp(o, P, 1), (2, 1)).out * k2 * sc)
    zu3 = conv3x3(o["a2"], r(P["conv.10.weight"]), P["conv.10.bias"]).out
    o["z3"] = r(zu3)
    keep_stats(2, zu3)
    H2 = o["z3"].shape[1]
    emb, n, sx, _, _ = time_mean(o["z3"], *_bnp(o, P, 2))
    o["emb"], o["msum"] = r32(emb), torch.stack([n, r32(sx)], dim=-1)
    o["logits"] = r32(F.linear(o["emb"].reshape(B, -1), P["classifier.weight"], P["classifier.bias"]).squeeze(-1))
    loss, dl = bce_smooth(o["logits"], o["y"])
    o["loss"], o["dlogits"] = float(loss), r32(dl)
    o["run"] = [((1 - MOMENTUM) * rm + MOMENTUM * o["mean"][l], (1 - MOMENTUM) * rv + MOMENTUM * o["var"][l] * (o["n"][l] / max(o["n"][l] - 1, 1)))
                for l, (rm, rv) in enumerate(o["run0"])]
    # ---- backward
    demb, g["classifier.weight"], g["classifier.bias"] = classifier_backward(o["dlogits"], o["emb"], P["classifier.weight"])
    o["demb"] = r32(demb)
    S1, S2 = saved_sums(o["demb"], o["msum"][..., 0], o["msum"][..., 1], H2)
    g["conv.11.bias"], g["conv.11.weight"] = r32(S1), r32(S2)
    up3 = (o["demb"] / H2).unsqueeze(1).expand(-1, H2, -1, -1)
    o["dz3"] = r(bn_bwd_apply(o["z3"], up3, *_bnp(o, P, 2), g["conv.11.bias"], g["conv.11.weight"], z_term=zu3 if autograd_xhat else None)[0].out)
    g["conv.10.weight"], g["conv.10.bias"] = conv3x3_wgrad(o["dz3"], o["a2"])
    o["da2"] = r(conv3x3_dgrad(o["dz3"], r(P["conv.10.weight"])).out)
    H1 = o["z2"].shape[1]
    up2 = upstream(o["da2"] * k2 * sc, H1, Fq, "pool21")
    red = bn_bwd_reduce(o["z2"], up2, *_bnp(o, P, 1))
    g["conv.6.bias"], g["conv.6.weight"] = r32(red.S1), r32(red.S2)
    o["dz2"] = r(bn_bwd_apply(o["z2"], up2, *_bnp(o, P, 1), g["conv.6.bias"], g["conv.6.weight"], z_term=zu2 if autograd_xhat else None)[0].out)
    g["conv.5.weight"], g["conv.5.bias"] = conv3x3_wgrad(o["dz2"], o["a1"])
    o["da1"] = r(conv3x3_dgrad(o["dz2"], r(P["conv.5.weight"])).out)           # (stored unmasked: the vector path's statement)
    b = block1_backward(x, w1, b1, gam, bet, mean, istd, o["da1"] * k1 * sc, src="pool21")
    g["conv.0.weight"], g["conv.0.bias"], g["conv.1.weight"], g["conv.1.bias"] = b.dW, b.db, b.dgamma, b.dbeta
    A, S1b, S2b, _ = block1_record(x, w1, b1, gam, bet, mean, istd, o["da1"] * k1 * sc)
    o["c1rec"] = torch.cat([r32(A), r32(S1b)[:, None], r32(S2b)[:, None]], dim=1)
    o["sums"] = [None, torch.stack([g["conv.6.bias"], g["conv.6.weight"]], dim=1), torch.stack([g["conv.11.bias"], g["conv.11.weight"]], dim=1)]
    return o


# -------------------------------------------------------------------------------------- every stage on one set of stored tensors
def read_keeps(o, sd, p):
    """The dropout keep masks of a step, read off its stored a1 and a2 (module docstring) -> ((keep1, keep2) bool, (determined1,
    determined2) bool: the elements whose undropped value exceeds its own allowance)"""
    P = _params(sd)
    sc = keep_scale(p)
    st1 = block1_forward(o["x"], P["conv.0.weight"], P["conv.0.bias"], *_bnp(o, P, 0)[2:], *_bnp(o, P, 0)[:2], F64, True, pool=(2, 1))
    st2 = bn_relu_pool(o["z2"], *_bnp(o, P, 1), (2, 1), F64, True)
    keeps, det = [], []
    for st, got in ((st1, o["a1"]), (st2, o["a2"])):
        d = st.out * sc > HALF_BF16 * st.out * sc + st.K * U * st.A * sc
        keeps.append(~((got == 0) & d))
        det.append(d)
    return tuple(keeps), tuple(det)


def stage_results(o, sd, dt=F64, mags=True, elem="bf16", fused=True, da1_masked=False, s2_derived=False):
    """Every stage evaluated in `dt` on the stored tensors `o` (the layout of run_chain's result; o["grads"] gives the sums the
    apply passes read, o["keep"] the dropout masks (1.0: none), o["p"] the rate) -> {stage name: Result}.  mags=False (the float32
    floor run): values only.  elem: the storage type of the activations ("bf16"; "fp32": they are held to the fp32 criterion and
    the convolutions take unrounded weights).  o["det"] (optional): read_keeps' determined elements.  Path: fused (the one-pass block-1 backward: XX | Xs and the [32][11] record exist),
    da1_masked (the data-gradient kernel applied layer 1's keep mask), s2_derived (the matrix-core record leaves S2 = 0)."""
    P = _params(sd)
    R = {}
    x, G = o["x"], o["grads"]
    B, T, Fq = x.shape
    p = o["p"]
    sc = keep_scale(p) if p > 0 else 1.0
    k1, k2 = o["keep"]
    wr = bf16 if elem == "bf16" else (lambda t: t)

    def el(st, factor=1.0, alt=None, amb=None, slack=None):
        """a stored activation: the bf16 criterion, or (fp32 mode) the fp32 one with an open decision's other branch as slack"""
        out = st.out * factor
        A = None if st.A is None else st.A * factor
        if elem == "bf16":
            return Result("bf16", out, A, st.K, alt, amb, slack)
        if mags and amb is not None:
            s = torch.where(amb, (alt.to(F64) - out.to(F64)).abs(), torch.zeros_like(out, dtype=F64))
            slack = s if slack is None else slack + s
        return Result("fp32", out, slack=slack)

    def put_stats(name, l, zsrc):
        m, v = batch_stats(zsrc, dt)
        n = zsrc.numel() // zsrc.shape[-1]
        R[name + ".mean"], R[name + ".var"] = Result("fp32", m), Result("fp32", v)
        R[name + ".invstd"] = Result("fp32", invstd_of(o["var"][l].to(dt)))             # (against the stored variance)
        rm, rv = P[BNL[l] + ".running_mean"].to(dt), P[BNL[l] + ".running_var"].to(dt)        # sd: the state before the step
        R[name + ".running_mean"] = Result("fp32", (1 - MOMENTUM) * rm + MOMENTUM * m)
        R[name + ".running_var"] = Result("fp32", (1 - MOMENTUM) * rv + MOMENTUM * v * (n / max(n - 1, 1)))
    w1, b1 = P["conv.0.weight"], P["conv.0.bias"]
    mean, istd, gam, bet = _bnp(o, P, 0)
    put_stats("b1", 0, conv3x3(x.unsqueeze(-1), w1, b1, dt).out)
    if fused:
        XX, Xs = tap_moments(x, dt)
        R["b1.XX"], R["b1.Xs"] = Result("fp32", XX), Result("fp32", Xs)
    R["b1.a"] = el(block1_forward(x, w1, b1, gam, bet, mean, istd, dt, mags, pool=(2, 1)), k1 * sc)
    zs = conv3x3(o["a1"], wr(P["conv.5.weight"]), P["conv.5.bias"], dt, mags)
    R["b2.z"] = el(zs)
    put_stats("b2", 1, zs.out)                                  # the unrounded accumulators, not the stored z2
    R["b2.a"] = el(bn_relu_pool(o["z2"], *_bnp(o, P, 1), (2, 1), dt, mags), k2 * sc)
    zs = conv3x3(o["a2"], wr(P["conv.10.weight"]), P["conv.10.bias"], dt, mags)
    R["b3.z"] = el(zs)
    put_stats("b3", 2, zs.out)
    H2, H1 = o["z3"].shape[1], o["z2"].shape[1]
    emb, n, sx, sl_n, sl_sx = time_mean(o["z3"], *_bnp(o, P, 2), dt)
    R["b3.emb"] = Result("fp32", emb)
    R["b3.msum.n"] = Result("fp32", n, slack=sl_n if mags else None, scale=1.0)          # counts: a deviation of one is 1.0
    R["b3.msum.sx"] = Result("fp32", sx, slack=sl_sx if mags else None)
    R["logits"] = Result("fp32", F.linear(o["emb"].to(dt).reshape(B, -1), P["classifier.weight"].to(dt), P["classifier.bias"].to(dt)).squeeze(-1))
    loss, dl = bce_smooth(o["logits"], o["y"], SMOOTHING, dt)
    R["bce.loss"], R["bce.dlogits"] = Result("fp32", loss.reshape(1)), Result("fp32", dl)
    # ---- backward
    demb, dWc, dbc = classifier_backward(o["dlogits"], o["emb"], P["classifier.weight"], dt)
    R["cls.demb"], R["classifier.weight"], R["classifier.bias"] = Result("fp32", demb), Result("fp32", dWc), Result("fp32", dbc)
    S1, S2 = saved_sums(o["demb"], o["msum"][..., 0], o["msum"][..., 1], H2, dt)
    R["conv.11.bias"], R["conv.11.weight"] = Result("fp32", S1), Result("fp32", S2)
    st3 = _bnp(o, P, 2)
    up3 = (o["demb"].to(dt) / H2).unsqueeze(1).expand(-1, H2, -1, -1)
    amb3 = bn_bwd_reduce(o["z3"], up3, *st3, dt).amb if mags else None
    ap, alt = bn_bwd_apply(o["z3"], up3, *st3, G["conv.11.bias"], G["conv.11.weight"], dt, mags)
    R["b3.dz"] = el(ap, alt=alt if mags else None, amb=amb3)
    dW, db = conv3x3_wgrad(o["dz3"], o["a2"], dt)
    R["conv.10.weight"] = Result("fp32", dW)
    R["conv.10.bias"] = Result("fp32", db, scale=float(o["dz3"].abs().sum(dim=(0, 1, 2)).max()))
    R["b3.dx"] = el(conv3x3_dgrad(o["dz3"], wr(P["conv.10.weight"]), dt, mags))
    st2 = _bnp(o, P, 1)
    up2 = upstream(o["da2"] * k2 * sc, H1, Fq, "pool21", dt)
    det1, det2 = o.get("det", (None, None))
    red = bn_bwd_reduce(o["z2"], up2, *st2, dt, also_open=open_rows(det2, H1))
    R["conv.6.weight"] = Result("fp32", red.S2, slack=red.slack2 if mags else None)
    R["conv.6.bias"] = Result("fp32", red.S1, slack=red.slack1 if mags else None)
    ap, alt = bn_bwd_apply(o["z2"], up2, *st2, G["conv.6.bias"], G["conv.6.weight"], dt, mags)
    if p > 0:       # the upstream gradient 0.5 ds da2 costs two roundings more on |up| <= A: the keep-scale 1 / (1 - p) and its product
        ap = Stage(ap.out, ap.A, ap.K + 2)
    R["b2.dz"] = el(ap, alt=alt if mags else None, amb=red.amb if mags else None)
    dW, db = conv3x3_wgrad(o["dz2"], o["a1"], dt)
    R["conv.5.weight"] = Result("fp32", dW)
    R["conv.5.bias"] = Result("fp32", db, scale=float(o["dz2"].abs().sum(dim=(0, 1, 2)).max()))
    dx = conv3x3_dgrad(o["dz2"], wr(P["conv.5.weight"]), dt, mags)
    if da1_masked:      # zero at dropped positions; an undetermined element (o["det"], read_keeps) may be stored either way: as stored
        R["b2.dx"] = el(dx, k1 if det1 is None else torch.where(det1, k1, (o["da1"] != 0).to(F64)))
    else:
        R["b2.dx"] = el(dx)
    da1s = o["da1"] * k1 * sc
    bk = block1_backward(x, w1, b1, gam, bet, mean, istd, da1s, dt, slack=mags, src="pool21", also_open=open_rows(det1, T))
    sl = bk.slack or {}
    R["conv.0.weight"] = Result("fp32", bk.dW, slack=sl.get("dW"))
    R["conv.0.bias"] = Result("fp32", bk.db, slack=sl.get("db"), scale=None if bk.db_terms is None else float(bk.db_terms.max()))
    R["conv.1.weight"] = Result("fp32", bk.dgamma, slack=sl.get("dgamma"))
    R["conv.1.bias"] = Result("fp32", bk.dbeta, slack=sl.get("dbeta"))
    if fused:
        A, S1b, S2b, rsl = block1_record(x, w1, b1, gam, bet, mean, istd, da1s, dt, slack=mags, also_open=open_rows(det1, T))
        rsl = rsl or (None, None, None)
        R["b1.rec.A"], R["b1.rec.S1"] = Result("fp32", A, slack=rsl[0]), Result("fp32", S1b, slack=rsl[1])
        if not s2_derived:
            R["b1.rec.S2"] = Result("fp32", S2b, slack=rsl[2])
    if mags:
        R["b1.relu"] = Result("share", torch.tensor(bk.amb_share))
    return R


STORED = {"b1.a": "a1", "b2.z": "z2", "b2.a": "a2", "b3.z": "z3", "b3.emb": "emb", "cls.demb": "demb", "b3.dz": "dz3", "b3.dx": "da2",
          "b2.dz": "dz2", "b2.dx": "da1", "b1.XX": "XX", "b1.Xs": "Xs", "logits": "logits", "bce.dlogits": "dlogits"}


def stored_of(o, name):
    """the stored counterpart of stage `name` in an operand set (None: that run stored none)"""
    if name in o["grads"]:
        return o["grads"][name]
    if name in STORED:
        return o.get(STORED[name])
    head, _, tail = name.partition(".")
    if tail in ("mean", "var", "invstd"):
        return o[tail][int(head[1]) - 1]
    if tail in ("running_mean", "running_var"):
        return o["run"][int(head[1]) - 1][tail == "running_var"]
    if name == "bce.loss":
        return torch.tensor([o["loss"]], dtype=F64)
    if name.startswith("b3.msum"):
        return o["msum"][..., 0 if tail == "msum.n" else 1]
    if name.startswith("b1.rec") and o.get("c1rec") is not None:
        return {"A": o["c1rec"][:, :9], "S1": o["c1rec"][:, 9], "S2": o["c1rec"][:, 10]}[name.rsplit(".", 1)[1]]
    return None
