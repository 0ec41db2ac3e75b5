"""Float64 statements of every kernel stage of the ConvAutoencoder's bf16 training step -- TEST INFRASTRUCTURE ONLY.

The model is the reference's src/model_cae.py:32-125 (four Conv2d 3x3 + BatchNorm + ReLU + AvgPool2d(2) blocks, three
ConvTranspose2d(k2, s2) + BatchNorm + ReLU blocks, the second with output_padding (0, 1), a last ConvTranspose2d 32 -> 1, zero
rows up to T); the rounding points are the ones oracle/torch_ref.py::cae_train_step_emulated documents.  Unlike that oracle no
stage here feeds another: each takes its operands as tensors, channels-last as the product stores them ([B, H, W, C]; weights in
torch's layouts), and returns what ONE kernel (or one kernel and its reduction) makes of them.  A test that hands every stage the
tensors the GPU itself stored therefore compares kernels one at a time; errors do not propagate and the conditioning of the
network does not enter.

Every stage runs in the arithmetic `dt` (float64: the statement; float32: the CPU's evaluation of the same stage, whose distance
from the float64 one is the floor of fp32 arithmetic).  With mags=True a stage also returns A, the float64 sum of the magnitudes
of the terms of each output element, and K, the number of roundings fp32 arithmetic spends on them, so that
K * 2^-24 * A bounds the error of any fp32 evaluation order (derivations at the stages).

Where the product's two directions use different weights the stage says which: the 3x3 convolutions (forward and data gradient)
and the ConvTranspose2d forward multiply by bf16(w); the ConvTranspose2d data gradient multiplies by bf16(w) on the matrix cores
(convt_dgrad_bf16.hip rounds its fragments RNE) and by the unrounded fp32 w in the fp32 GEMM path (option cae_dgrad_mfma = 0);
block 1 and decoder block 4 use fp32 weights; every weight gradient is a product of the two stored tensors.

`run_chain` strings the stages together (float64, roundings on or off) -- that is how the CPU tests pin this file against
oracle/torch_ref.py and make operands; `stage_results` evaluates every stage on a given set of stored tensors; `compare` holds a
set of results to the criteria of tests/test_cae_train_stages_gpu.py.
"""
from collections import namedtuple

import numpy as np
import torch
import torch.nn.functional as F

F64, F32 = torch.float64, torch.float32
U = 2.0 ** -24                   # unit roundoff of fp32
HALF_BF16 = 2.0 ** -8            # half a bf16 step, relative to the value (worst case: the bottom of a binade)
BN_EPS = 1e-5
ENC_C, DEC_C, DEC_CIN = (32, 64, 128, 256), (128, 64, 32), (256, 128, 64)
ENC_IDX, DEC_IDX = ((0, 1), (4, 5), (8, 9), (12, 13)), ((0, 1), (3, 4), (6, 7))       # (conv, BatchNorm) of the nn.Sequentials
PARAM_ORDER = [f"encoder.{i}.{k}" for c, b in ENC_IDX for i in (c, b) for k in ("weight", "bias")] + \
              [f"decoder.{i}.{k}" for c, b in DEC_IDX for i in (c, b) for k in ("weight", "bias")] + \
              ["decoder.9.weight", "decoder.9.bias"]
K_BN = 8          # fp32 roundings of one BatchNorm output gamma * invstd * (z - mean) + beta, whichever way it is associated (below)
K_BLOCK1 = 24     # ... of one block-1 BatchNorm output formed from x: 9 taps + bias through the folded image (below)

Stage = namedtuple("Stage", "out A K")

# The cases of tests/test_cae_train_stages_gpu.py (tests/test_cae_train_stages_cpu.py runs the float32 CPU stages on every one):
# the smallest shape the ABI takes (latent 1x1); latent height 1 (the shape of the overwritten-statistics bug); odd at every
# level (twice); T = 33; the real shape (a dropped row, a zero tail row, six strips); odd 161 -> 80; 15 zero tail rows
CASES = [(1, 16, 20), (2, 17, 20), (3, 31, 36), (2, 47, 52), (2, 33, 20), (2, 321, 180), (3, 322, 180), (2, 335, 180)]


def ordinary_state(seed):
    """state_dict of a default-initialised ConvAutoencoder with gamma uniform in [0.5, 1.5] and beta = 0.1 randn"""
    from dfa_amd.model_cae import ConvAutoencoder
    torch.manual_seed(seed)
    m = ConvAutoencoder()
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for seq, idx in ((m.encoder, ENC_IDX), (m.decoder, DEC_IDX)):
            for _, b in idx:
                seq[b].weight.copy_(0.5 + torch.rand(seq[b].weight.shape, generator=g))
                seq[b].bias.copy_(0.1 * torch.randn(seq[b].bias.shape, generator=g))
    return {k: v.detach().clone() for k, v in m.state_dict().items()}


def case_input(B, T, F_, seed=None):
    """x [B,T,F] = randn (the auto-encoder sees z-scored features), float32"""
    return torch.randn(B, T, F_, generator=torch.Generator().manual_seed(1000 + B + T + F_ if seed is None else seed))


def bf16(t):
    """round to bf16 (through fp32, as the kernels' fp32 accumulators are), keeping the dtype"""
    return t.to(F32).to(torch.bfloat16).to(t.dtype)


def f32r(t):
    return t.to(F32).to(t.dtype)


def _nchw(t):
    return t.permute(0, 3, 1, 2)


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


# ---------------------------------------------------------------------------------------------------------- forward stages
def conv3x3(a, w, b, dt=F64, mags=False):
    """a [B,H,W,Cin], w [Cout,Cin,3,3], b [Cout] -> the unrounded pre-BatchNorm output [B,H,W,Cout] (zero padding 1).
    K = 9 Cin + 1 terms summed in fp32: (K - 1) roundings."""
    a_, w_, b_ = _nchw(a.to(dt)), w.to(dt), b.to(dt)
    out = _nhwc(F.conv2d(a_, w_, b_, padding=1))
    A = _nhwc(F.conv2d(a_.abs(), w_.abs(), b_.abs(), padding=1)) if mags else None
    return Stage(out, A, 9 * w.shape[1] + 1)


def convt2x2(a, w, b, opad=0, dt=F64, mags=False):
    """ConvTranspose2d(k2, s2): a [B,H,W,Cin], w [Cin,Cout,2,2], b [Cout] -> [B,2H,2W+opad,Cout]; the output_padding column has
    no input pixel and holds the bias.  K = Cin + 1."""
    a_, w_, b_ = _nchw(a.to(dt)), w.to(dt), b.to(dt)
    out = _nhwc(F.conv_transpose2d(a_, w_, b_, stride=2, output_padding=(0, opad)))
    A = _nhwc(F.conv_transpose2d(a_.abs(), w_.abs(), b_.abs(), stride=2, output_padding=(0, opad))) if mags else None
    return Stage(out, A, w.shape[0] + 1)


def batch_stats(z, dt=F64, valid=None):
    """(mean, biased variance) over batch and pixels of z [B,H,W,C]; valid (bool, broadcastable to z): over those pixels only (the
    frames of a ragged batch's utterances; what z holds elsewhere is not read)"""
    z = z.to(dt)
    if valid is not None:
        z = torch.where(valid, z, torch.zeros_like(z))
        n = valid.expand(z.shape).to(dt).sum(dim=(0, 1, 2))
        mean = z.sum(dim=(0, 1, 2)) / n
        return mean, torch.where(valid, (z - mean) ** 2, torch.zeros_like(z)).sum(dim=(0, 1, 2)) / n
    mean = z.mean(dim=(0, 1, 2))
    return mean, ((z - mean) ** 2).mean(dim=(0, 1, 2))


def invstd_of(var):
    return 1.0 / torch.sqrt(var + BN_EPS)


def _pool22(t):
    H2, W2 = t.shape[1] // 2, t.shape[2] // 2
    t = t[:, :2 * H2, :2 * W2]
    return 0.25 * ((t[:, 0::2, 0::2] + t[:, 1::2, 0::2]) + (t[:, 0::2, 1::2] + t[:, 1::2, 1::2]))


def _pool21(t):
    H2 = t.shape[1] // 2
    return 0.5 * (t[:, 0:2 * H2:2] + t[:, 1:2 * H2:2])


def _pool(t, pool):
    return _pool22(t) if pool == 2 else _pool21(t) if pool == (2, 1) else t


def bn_relu_pool(z, mean, invstd, gamma, beta, pool, dt=F64, mags=False):
    """z [B,H,W,C] (as stored), the layer's statistics and affine parameters -> ReLU(BatchNorm(z)), averaged over 2x2 windows when
    pool == 2 and over row pairs when pool == (2, 1) (floor: a last odd row / column is dropped).
    Error of one BatchNorm output y in fp32, for A_y = |z s| + |mean s| + |beta|, s = gamma invstd: s costs one rounding (u A_y on
    the first two terms), shift = beta - mean s two more on its product and one on the difference (<= 3u A_y), the fused
    multiply-add one (u |y| <= u A_y); the same count holds for (z - mean) invstd gamma + beta.  <= 6u A_y, K_BN = 8 leaves room
    for the stored invstd's own rounding.  ReLU is 1-Lipschitz, the pool's three additions cost 3u of their sum: K = K_BN + 4."""
    z, mean, invstd, gamma, beta = (t.to(dt) for t in (z, mean, invstd, gamma, beta))
    s = gamma * invstd
    r = F.relu((z - mean) * s + beta)
    out = _pool(r, pool)
    A = None
    if mags:
        a = (z * s).abs() + (mean * s).abs() + beta.abs()
        A = _pool(a, pool)
    return Stage(out, A, K_BN + (4 if pool != 1 else 0))


def block1_forward(x, w, b, gamma, beta, mean, invstd, dt=F64, mags=False, pool=2):
    """x [B,T,F], the fp32 block-1 parameters and ITS batch statistics -> e[0] = pool(ReLU(BatchNorm(conv(x)))) [B,T/2,F/2,32]
    (pool = (2, 1): row pairs only, [B,T/2,F,32]).
    The kernels fold the statistics into the weights first (fw = w s, fb = (b - mean) s + beta; three roundings each), then sum
    nine products and the bias (vector path: fused multiply-adds; matrix-core path: the three-term bf16 split of fw, exact to
    2^-24 per product): <= (3 + 10 + 3 + 3) u A_y with A_y = s (sum |x w| + |b| + |mean|) + |beta|; K_BLOCK1 = 24 with the pool."""
    zs = conv3x3(x.unsqueeze(-1), w, b, dt, mags)
    st = bn_relu_pool(zs.out, mean, invstd, gamma, beta, pool, dt)
    A = None
    if mags:
        s = (gamma.to(dt) * invstd.to(dt)).abs()
        A = _pool(s * (zs.A + mean.to(dt).abs()) + beta.to(dt).abs(), pool)
    return Stage(st.out, A, K_BLOCK1)


def dec4_forward(d2, w, b, x, dt=F64):
    """d[2] [B,H3,W3,32], decoder.9 (fp32), x [B,T,F] -> (reconstruction [B,T,F] with zero rows past 2 H3, per-sample MSE [B])"""
    r = convt2x2(d2, w, b, 0, dt).out[..., 0]
    T = x.shape[1]
    recon = F.pad(r, (0, 0, 0, T - r.shape[1])) if r.shape[1] < T else r[:, :T]
    return recon, ((recon - x.to(dt)) ** 2).mean(dim=(1, 2))


# --------------------------------------------------------------------------------------------------------- backward stages
def dec4_backward(d2, w, b, x, drecon=None, dt=F64, mags=False):
    """Decoder block 4: g = drecon, or 2 (recon - x) / (B T F) recomputed from d[2] (the loss is MSELoss(recon, x); the zero tail
    rows carry no gradient) -> (Stage dd[2] [B,H3,W3,32], dW [32,1,2,2], db [1]).
    dd[2] = sum_q g_q w_q.  In the MSE form g_q = scale (b + sum_ci d w - x) costs 35 roundings of G_q = scale (sum |d w| + |b| +
    |x|), the four products and three additions 4 more of sum |g_q w_q| <= sum |w_q| G_q =: A; K = 40."""
    d2_, w_, b_ = d2.to(dt), w.to(dt), b.to(dt)
    B, H3, W3, _ = d2.shape
    T, Fq = x.shape[1], x.shape[2]
    rows = min(2 * H3, T)
    if drecon is None:
        scale = 2.0 / (B * T * Fq)
        r = convt2x2(d2, w, b, 0, dt).out[..., 0]
        g = scale * (r - x.to(dt)[:, :2 * H3])
    else:
        g = drecon.to(dt)[:, :2 * H3].clone()
    g[:, rows:] = 0
    dd = _nhwc(F.conv2d(g.unsqueeze(1), w_, stride=2))
    d2f = d2_.reshape(-1, 32)
    dW = torch.stack([d2f.T @ g[:, a::2, c::2].reshape(-1) for a in (0, 1) for c in (0, 1)], dim=1).reshape(32, 1, 2, 2)
    db = g.sum().reshape(1)
    A, K = None, 4
    if mags:
        if drecon is None:
            G = scale * (convt2x2(d2.abs(), w.abs(), b.abs(), 0, F64).out[..., 0] + x.to(F64)[:, :2 * H3].abs())
            K = 40
        else:
            G = g.to(F64).abs()
        A = _nhwc(F.conv2d(G.unsqueeze(1), w.to(F64).abs(), stride=2))
    return Stage(dd, A, K), dW, db


def upstream(da, H, W, src, dt=F64):
    """the gradient that arrives at a BatchNorm + ReLU output [B,H,W,C]: da itself ("direct": the decoder), a quarter of da at
    each of a pooled window's four pixels and zero on a dropped last row / column ("pool22": the encoder), or half of da at each
    row of a pooled pair and zero on a dropped last row ("pool21")"""
    da = da.to(dt)
    if src == "direct":
        return da
    up = torch.zeros((da.shape[0], H, W, da.shape[3]), dtype=dt)
    if src == "pool21":
        up[:, :2 * (H // 2)] = 0.5 * da.repeat_interleave(2, dim=1)
        return up
    up[:, :2 * (H // 2), :2 * (W // 2)] = 0.25 * da.repeat_interleave(2, dim=1).repeat_interleave(2, dim=2)
    return up


BnReduce = namedtuple("BnReduce", "S1 S2 slack1 slack2 on amb xh")


def bn_bwd_reduce(z, up, mean, invstd, gamma, beta, dt=F64, k_amb=K_BN, terms=None, also_open=None, valid=None):
    """z as stored, `up` = upstream(...) -> S1 = sum dy (dbeta), S2 = sum dy xhat (dgamma) with dy = up where BatchNorm(z) > 0.
    amb marks the elements whose BatchNorm output y lies within k_amb u (|gamma| invstd (|z| + |mean|) + |beta|) of zero -- the
    fp32 rounding of its own terms (`terms`: the caller's own sum of magnitudes, block 1) -- so that an fp32 kernel may take
    either branch; slack1 / slack2 are what those elements can move the two sums by (sum |up|, sum |up xhat| over them).
    also_open: elements whose dy the caller cannot state wherever their ReLU is on (a bool mask; and-ed with `on`, or-ed into amb).
    valid (bool, broadcastable to z): the elements that belong to the batch (a ragged batch's own frames); `up` is zero at the others,
    which are no decisions: amb is and-ed with it."""
    z, up, mean, invstd, gamma, beta = (t.to(dt) for t in (z, up, mean, invstd, gamma, beta))
    xh = (z - mean) * invstd
    y = gamma * xh + beta
    on = y > 0
    dy = torch.where(on, up, torch.zeros_like(up))
    if terms is None:
        terms = gamma.abs() * invstd * (z.abs() + mean.abs()) + beta.abs()
    amb = y.abs() <= k_amb * U * terms.to(dt)
    if also_open is not None:
        amb = amb | (also_open & on)
    if valid is not None:
        amb = amb & valid
    au = up.abs() * amb
    return BnReduce(dy.sum(dim=(0, 1, 2)), (dy * xh).sum(dim=(0, 1, 2)), au.sum(dim=(0, 1, 2)), (au * xh.abs()).sum(dim=(0, 1, 2)),
                    on, amb, xh)


def bn_bwd_apply(z, up, mean, invstd, gamma, beta, S1, S2, dt=F64, mags=False, z_term=None, n=None):
    """dz = gamma invstd (dy - S1 / N - xhat S2 / N) with the sums the caller gives (the GPU's own) -> (Stage dz, dz with the ReLU
    decision of every element reversed).  k0 = gamma invstd, k1, k2 one rounding each, xhat two, the bracket three, the product
    one: K = K_BN of A = |k0| (|up| + |k1| + invstd (|z| + |mean|) |k2|).  z_term: the tensor the xhat of the S2 term is formed
    from when it is not z (autograd through statistics of the unrounded accumulators; the kernels take z).  n: the count the
    statistics ran over when it is not every pixel of z (the frames of a ragged batch)."""
    z, up, mean, invstd, gamma, beta, S1, S2 = (t.to(dt) for t in (z, up, mean, invstd, gamma, beta, S1, S2))
    N = z.shape[0] * z.shape[1] * z.shape[2] if n is None else n
    k0, k1, k2 = gamma * invstd, S1 / N, S2 / N
    xh = (z - mean) * invstd
    on = (gamma * xh + beta) > 0
    if z_term is not None:
        xh = (z_term.to(dt) - mean) * invstd
    off_v = k0 * (-k1 - xh * k2)
    on_v = k0 * (up - k1 - xh * k2)
    A = (k0.abs() * (up.abs() + k1.abs() + invstd * (z.abs() + mean.abs()) * k2.abs())) if mags else None
    return Stage(torch.where(on, on_v, off_v), A, K_BN), torch.where(on, off_v, on_v)


def conv3x3_wgrad(dz, a, dt=F64):
    """dz [B,H,W,Cout], the layer's input a [B,H,W,Cin] -> (dW [Cout,Cin,3,3], db [Cout] = the channel sums of dz)"""
    B, H, W, Co = dz.shape
    Ci = a.shape[3]
    ap = F.pad(a.to(dt), (0, 0, 1, 1, 1, 1))
    dzf = dz.to(dt).reshape(-1, Co)
    dW = torch.empty((Co, Ci, 3, 3), dtype=dt)
    for ky in range(3):
        for kx in range(3):
            dW[:, :, ky, kx] = dzf.T @ ap[:, ky:ky + H, kx:kx + W].reshape(-1, Ci)
    return dW, dzf.sum(dim=0)


def conv3x3_dgrad(dz, w, dt=F64, mags=False):
    """dz [B,H,W,Cout], w [Cout,Cin,3,3] -> the gradient of the layer's input [B,H,W,Cin]; K = 9 Cout terms"""
    dz_, w_ = _nchw(dz.to(dt)), w.to(dt)
    out = _nhwc(F.conv_transpose2d(dz_, w_, padding=1))
    A = _nhwc(F.conv_transpose2d(dz_.abs(), w_.abs(), padding=1)) if mags else None
    return Stage(out, A, 9 * w.shape[0])


def convt_dgrad(dzd, w, dt=F64, mags=False):
    """dzd [B,2H,2W+opad,Cout], w [Cin,Cout,2,2] -> the gradient of the layer's input [B,H,W,Cin] (an output_padding column has no
    input pixel and does not enter); K = 4 Cout terms"""
    dz_, w_ = _nchw(dzd.to(dt)), w.to(dt)
    out = _nhwc(F.conv2d(dz_, w_, stride=2))
    A = _nhwc(F.conv2d(dz_.abs(), w_.abs(), stride=2)) if mags else None
    return Stage(out, A, 4 * w.shape[1])


def convt_wgrad(a, dzd, dt=F64):
    """the layer's input a [B,H,W,Cin], dzd [B,2H,2W+opad,Cout] -> (dW [Cin,Cout,2,2], db [Cout] = the channel sums of dzd over ALL
    output pixels, the output_padding column included)"""
    B, H, W, Ci = a.shape
    Co = dzd.shape[3]
    af, dz_ = a.to(dt).reshape(-1, Ci), dzd.to(dt)
    dW = torch.empty((Ci, Co, 2, 2), dtype=dt)
    for p in (0, 1):
        for q in (0, 1):
            dW[:, :, p, q] = af.T @ dz_[:, p:2 * H:2, q:2 * W:2].reshape(-1, Co)
    return dW, dz_.sum(dim=(0, 1, 2))


Block1Bwd = namedtuple("Block1Bwd", "dW db dgamma dbeta slack amb_share db_terms")


def block1_backward(x, w, b, gamma, beta, mean, invstd, de0, dt=F64, slack=False, src="pool22", also_open=None):
    """x [B,T,F], block 1's fp32 parameters and statistics, de[0] [B,T/2,F/2,32] -> the block's four gradients.  Its pre-BatchNorm
    output is recomputed, never stored, so the ReLU decisions are the stage's own: with slack=True the result carries, per
    gradient, what the elements within K_BLOCK1 roundings of zero could move it by (the gradients are linear in dy: the magnitudes
    |up| of those elements are sent through the same sums with every factor replaced by its magnitude), their share, and the sum
    of magnitudes of the bias gradient's terms (that gradient is a sum that cancels to rounding noise: it is measured against
    its terms, not against itself)."""
    B, T, Fq = x.shape
    x4 = x.unsqueeze(-1)
    zs = conv3x3(x4, w, b, dt, mags=slack)
    up = upstream(de0, T, Fq, src, dt)
    terms = None
    if slack:
        terms = (gamma * invstd).abs() * (zs.A + mean.abs()) + beta.abs()
    red = bn_bwd_reduce(zs.out, up, mean, invstd, gamma, beta, dt, K_BLOCK1, terms, also_open)
    dz = bn_bwd_apply(zs.out, up, mean, invstd, gamma, beta, red.S1, red.S2, dt)[0].out
    dW, db = conv3x3_wgrad(dz, x4, dt)
    sl, share, dbt = None, None, None
    if slack:
        N = B * T * Fq
        k0 = (gamma * invstd).abs().to(dt)
        dza = k0 * (up.abs() * red.amb + red.slack1 / N + red.xh.abs() * red.slack2 / N)
        sW, sb = conv3x3_wgrad(dza, x4.abs(), dt)
        sl = {"dW": sW, "db": sb, "dgamma": red.slack2, "dbeta": red.slack1}
        share = float(red.amb.double().mean())
        dbt = dz.abs().sum(dim=(0, 1, 2))
    return Block1Bwd(dW, db, red.S2, red.S1, sl, share, dbt)


# ------------------------------------------------------------------------------------------------------------------ the chain
def _params(sd, dt=F64):
    return {k: (v if isinstance(v, torch.Tensor) else torch.from_numpy(np.asarray(v))).detach().cpu().to(dt) for k, v in sd.items()
            if k in PARAM_ORDER}


def run_chain(sd, x, rounding=True, stats="epilogue", dgrad_bf16=True):
    """One training step as a chain of the stages above in float64.  rounding=False: no rounding anywhere (must equal
    cae_train_step_emulated(emulate=None)).  rounding=True: every tensor the product stores in bf16 is rounded where it is stored,
    the matrix-core layers take bf16 weights, statistics and sums are kept in fp32, and the batch statistics of encoder blocks 2-3
    and of the decoder come from the unrounded outputs (stats="epilogue") or from the stored ones ("stored"; block 4 always).
    -> dict: x, e[4], z[4] (z[0] None), zd[3], d[3], dd[3], dzd[3], de[4], dz[4], mean[7], var[7], invstd[7], recon, mse, loss, grads."""
    P = _params(sd)
    r = bf16 if rounding else (lambda t: t)
    r32 = f32r if rounding else (lambda t: t)
    x = r(x.detach().cpu().to(F64))
    o = {"x": x, "e": [None] * 4, "z": [None] * 4, "zd": [None] * 3, "d": [None] * 3, "dd": [None] * 3, "dzd": [None] * 3,
         "de": [None] * 4, "dz": [None] * 4, "mean": [None] * 7, "var": [None] * 7, "invstd": [None] * 7, "grads": {}}
    g = o["grads"]

    def keep_stats(i, zsrc):
        m, v = batch_stats(zsrc)
        o["mean"][i], o["var"][i], o["invstd"][i] = r32(m), r32(v), r32(invstd_of(v))

    def bn(i, pfx):
        return o["mean"][i], o["invstd"][i], P[pfx + ".weight"], P[pfx + ".bias"]
    c, bnk = ENC_IDX[0]
    keep_stats(0, conv3x3(x.unsqueeze(-1), P[f"encoder.{c}.weight"], P[f"encoder.{c}.bias"]).out)
    mean, istd, gam, bet = bn(0, f"encoder.{bnk}")
    o["e"][0] = r(block1_forward(x, P[f"encoder.{c}.weight"], P[f"encoder.{c}.bias"], gam, bet, mean, istd).out)
    for l in range(1, 4):
        c, bnk = ENC_IDX[l]
        zu = conv3x3(o["e"][l - 1], r(P[f"encoder.{c}.weight"]), P[f"encoder.{c}.bias"]).out
        o["z"][l] = r(zu)
        keep_stats(l, zu if (stats == "epilogue" and l < 3) else o["z"][l])
        o["e"][l] = r(bn_relu_pool(o["z"][l], *bn(l, f"encoder.{bnk}"), 2).out)
    for l in range(3):
        c, bnk = DEC_IDX[l]
        src = o["e"][3] if l == 0 else o["d"][l - 1]
        zu = convt2x2(src, r(P[f"decoder.{c}.weight"]), P[f"decoder.{c}.bias"], 1 if l == 1 else 0).out
        o["zd"][l] = r(zu)
        keep_stats(4 + l, zu if stats == "epilogue" else o["zd"][l])
        o["d"][l] = r(bn_relu_pool(o["zd"][l], *bn(4 + l, f"decoder.{bnk}"), 1).out)
    o["recon"], o["mse"] = dec4_forward(o["d"][2], P["decoder.9.weight"], P["decoder.9.bias"], x)
    o["loss"] = float(o["mse"].mean())
    # ---- backward
    st, g["decoder.9.weight"], g["decoder.9.bias"] = dec4_backward(o["d"][2], P["decoder.9.weight"], P["decoder.9.bias"], x)
    o["dd"][2] = r(st.out)
    for l in (2, 1, 0):
        c, bnk = DEC_IDX[l]
        src = o["e"][3] if l == 0 else o["d"][l - 1]
        stt = bn(4 + l, f"decoder.{bnk}")
        red = bn_bwd_reduce(o["zd"][l], o["dd"][l], *stt)
        g[f"decoder.{bnk}.weight"], g[f"decoder.{bnk}.bias"] = r32(red.S2), r32(red.S1)
        o["dzd"][l] = r(bn_bwd_apply(o["zd"][l], o["dd"][l], *stt, g[f"decoder.{bnk}.bias"], g[f"decoder.{bnk}.weight"])[0].out)
        w = P[f"decoder.{c}.weight"]
        dx = r(convt_dgrad(o["dzd"][l], r(w) if dgrad_bf16 else w).out)
        if l == 0:
            o["de"][3] = dx
        else:
            o["dd"][l - 1] = dx
        g[f"decoder.{c}.weight"], g[f"decoder.{c}.bias"] = convt_wgrad(src, o["dzd"][l])
    for l in (3, 2, 1):
        c, bnk = ENC_IDX[l]
        stt = bn(l, f"encoder.{bnk}")
        H, W = o["z"][l].shape[1:3]
        up = upstream(o["de"][l], H, W, "pool22")
        red = bn_bwd_reduce(o["z"][l], up, *stt)
        g[f"encoder.{bnk}.weight"], g[f"encoder.{bnk}.bias"] = r32(red.S2), r32(red.S1)
        o["dz"][l] = r(bn_bwd_apply(o["z"][l], up, *stt, g[f"encoder.{bnk}.bias"], g[f"encoder.{bnk}.weight"])[0].out)
        g[f"encoder.{c}.weight"], g[f"encoder.{c}.bias"] = conv3x3_wgrad(o["dz"][l], o["e"][l - 1])
        o["de"][l - 1] = r(conv3x3_dgrad(o["dz"][l], r(P[f"encoder.{c}.weight"])).out)
    c, bnk = ENC_IDX[0]
    b1 = block1_backward(x, P[f"encoder.{c}.weight"], P[f"encoder.{c}.bias"], gam, bet, mean, istd, o["de"][0])
    g[f"encoder.{c}.weight"], g[f"encoder.{c}.bias"], g[f"encoder.{bnk}.weight"], g[f"encoder.{bnk}.bias"] = b1.dW, b1.db, b1.dgamma, b1.dbeta
    return o


# -------------------------------------------------------------------------------------- every stage on one set of stored tensors
# kind "bf16": a tensor stored in bf16 (out = the unrounded statement; A, K its fp32 bound; alt / amb: the other ReLU branch and
# where it may be taken; eslack: an absolute allowance per element, used where an operand could only be restated);
# kind "fp32": an fp32 output (slack: absolute allowance per element from ambiguous ReLU decisions or restated operands; scale:
# the tensor's scale when it is not max |want|)
# kind "allow": an output held to a derived absolute allowance per element (slack) alone -- worst = max |got - want| / slack, bound 1
Result = namedtuple("Result", "kind out A K alt amb slack scale", defaults=(None,) * 6)


def stage_results(ops, sd, dt=F64, full=True, stats="epilogue", dgrad_bf16=True, have_dzd=(True, True, True)):
    """Every stage evaluated in `dt` on the stored tensors `ops` (the layout of run_chain's result; ops["grads"] gives the BatchNorm
    sums S1 = d beta, S2 = d gamma the apply passes read) -> {stage name: Result}.  full=False (the float32 floor run): values
    only.  stats: where the statistics of encoder blocks 2-3 and the decoder are summed from.  have_dzd[l] False: dzd[l] was never
    stored (the folded BatchNorm-backward pass): it is restated as bf16(float64 dzd) from zd, dd and the sums, and its consumers
    carry the allowance E = |bf16(want) - want| + K u A (+ the other ReLU branch where ambiguous) sent through their own sums."""
    P = _params(sd)
    R = {}
    x = ops["x"]
    G = ops["grads"]
    mg = full

    def bnp(i, pfx):
        return ops["mean"][i], ops["invstd"][i], P[pfx + ".weight"], P[pfx + ".bias"]

    def put_stats(name, i, zsrc):
        m, v = batch_stats(zsrc, dt)
        R[name + ".mean"], R[name + ".var"] = Result("fp32", m), Result("fp32", v)
        # (the stored inverse standard deviation against the stored variance)
        R[name + ".invstd"] = Result("fp32", invstd_of(ops["var"][i].to(dt)))
    c, bnk = ENC_IDX[0]
    w1, b1 = P[f"encoder.{c}.weight"], P[f"encoder.{c}.bias"]
    put_stats("enc1", 0, conv3x3(x.unsqueeze(-1), w1, b1, dt).out)
    R["enc1.e"] = Result("bf16", *block1_forward(x, w1, b1, *bnp(0, f"encoder.{bnk}")[2:], *bnp(0, f"encoder.{bnk}")[:2], dt, mg))
    for l in range(1, 4):
        c, bnk = ENC_IDX[l]
        zs = conv3x3(ops["e"][l - 1], bf16(P[f"encoder.{c}.weight"]), P[f"encoder.{c}.bias"], dt, mg)
        R[f"enc{l + 1}.z"] = Result("bf16", *zs)
        put_stats(f"enc{l + 1}", l, zs.out if (stats == "epilogue" and l < 3) else ops["z"][l])
        R[f"enc{l + 1}.e"] = Result("bf16", *bn_relu_pool(ops["z"][l], *bnp(l, f"encoder.{bnk}"), 2, dt, mg))
    for l in range(3):
        c, bnk = DEC_IDX[l]
        src = ops["e"][3] if l == 0 else ops["d"][l - 1]
        zs = convt2x2(src, bf16(P[f"decoder.{c}.weight"]), P[f"decoder.{c}.bias"], 1 if l == 1 else 0, dt, mg)
        R[f"dec{l + 1}.zd"] = Result("bf16", *zs)
        put_stats(f"dec{l + 1}", 4 + l, zs.out if stats == "epilogue" else ops["zd"][l])
        R[f"dec{l + 1}.d"] = Result("bf16", *bn_relu_pool(ops["zd"][l], *bnp(4 + l, f"decoder.{bnk}"), 1, dt, mg))
    recon, mse = dec4_forward(ops["d"][2], P["decoder.9.weight"], P["decoder.9.bias"], x, dt)
    R["dec4.recon"], R["dec4.mse"] = Result("fp32", recon), Result("fp32", mse)
    # ---- backward
    st, dW, db = dec4_backward(ops["d"][2], P["decoder.9.weight"], P["decoder.9.bias"], x, None, dt, mg)
    R["dec4.dd"], R["decoder.9.weight"], R["decoder.9.bias"] = Result("bf16", *st), Result("fp32", dW), Result("fp32", db)
    for l in (2, 1, 0):
        c, bnk = DEC_IDX[l]
        src = ops["e"][3] if l == 0 else ops["d"][l - 1]
        stt = bnp(4 + l, f"decoder.{bnk}")
        red = bn_bwd_reduce(ops["zd"][l], ops["dd"][l], *stt, dt)
        R[f"decoder.{bnk}.weight"] = Result("fp32", red.S2, slack=red.slack2 if mg else None)
        R[f"decoder.{bnk}.bias"] = Result("fp32", red.S1, slack=red.slack1 if mg else None)
        ap, alt = bn_bwd_apply(ops["zd"][l], ops["dd"][l], *stt, G[f"decoder.{bnk}.bias"], G[f"decoder.{bnk}.weight"], dt, mg)
        w = P[f"decoder.{c}.weight"]
        wd = bf16(w) if dgrad_bf16 else w
        E = None
        if have_dzd[l]:
            R[f"dec{l + 1}.dzd"] = Result("bf16", *ap, alt=alt if mg else None, amb=red.amb if mg else None)
            dzd = ops["dzd"][l]
        else:
            dzd = bf16(ap.out)
            if mg:
                E = (dzd - ap.out).abs() + ap.K * U * ap.A + torch.where(red.amb, (alt - ap.out).abs(), torch.zeros_like(alt))
        dx = convt_dgrad(dzd, wd, dt, mg)
        dWt, dbt = convt_wgrad(src, dzd, dt)
        sx = sW = sb = None
        if E is not None:
            sx = convt_dgrad(E, wd.abs(), F64).out
            sW, sb = convt_wgrad(src.abs(), E, F64)
        R[f"dec{l + 1}.dx"] = Result("bf16", *dx, slack=sx)
        R[f"decoder.{c}.weight"], R[f"decoder.{c}.bias"] = Result("fp32", dWt, slack=sW), Result("fp32", dbt, slack=sb)
    for l in (3, 2, 1):
        c, bnk = ENC_IDX[l]
        stt = bnp(l, f"encoder.{bnk}")
        H, W = ops["z"][l].shape[1:3]
        up = upstream(ops["de"][l], H, W, "pool22", dt)
        red = bn_bwd_reduce(ops["z"][l], up, *stt, dt)
        R[f"encoder.{bnk}.weight"] = Result("fp32", red.S2, slack=red.slack2 if mg else None)
        R[f"encoder.{bnk}.bias"] = Result("fp32", red.S1, slack=red.slack1 if mg else None)
        ap, alt = bn_bwd_apply(ops["z"][l], up, *stt, G[f"encoder.{bnk}.bias"], G[f"encoder.{bnk}.weight"], dt, mg)
        R[f"enc{l + 1}.dz"] = Result("bf16", *ap, alt=alt if mg else None, amb=red.amb if mg else None)
        dWc, dbc = conv3x3_wgrad(ops["dz"][l], ops["e"][l - 1], dt)
        R[f"encoder.{c}.weight"], R[f"encoder.{c}.bias"] = Result("fp32", dWc), Result("fp32", dbc)
        R[f"enc{l + 1}.dx"] = Result("bf16", *conv3x3_dgrad(ops["dz"][l], bf16(P[f"encoder.{c}.weight"]), dt, mg))
    c, bnk = ENC_IDX[0]
    mean, istd, gam, bet = bnp(0, f"encoder.{bnk}")
    b = block1_backward(x, w1, b1, gam, bet, mean, istd, ops["de"][0], dt, slack=mg)
    sl = b.slack or {}
    R[f"encoder.{c}.weight"] = Result("fp32", b.dW, slack=sl.get("dW"))
    R[f"encoder.{c}.bias"] = Result("fp32", b.db, slack=sl.get("db"), scale=None if b.db_terms is None else float(b.db_terms.max()))
    R[f"encoder.{bnk}.weight"] = Result("fp32", b.dgamma, slack=sl.get("dgamma"))
    R[f"encoder.{bnk}.bias"] = Result("fp32", b.dbeta, slack=sl.get("dbeta"))
    if mg:
        R["enc1.relu"] = Result("share", torch.tensor(b.amb_share))
    return R


# what the GPU stored for each stage: name -> how to read it out of an operand set
def stored_of(ops, name):
    """the stored counterpart of stage `name` in an operand set (None: that run stored none)"""
    head, _, tail = name.partition(".")
    if name in ops["grads"]:
        return ops["grads"][name]
    i = int(head[3:]) - 1
    if head.startswith("enc"):
        if tail in ("mean", "var", "invstd"):
            return ops[tail][i]
        return {"e": ops["e"][i], "z": ops["z"][i], "dz": ops["dz"][i], "dx": ops["de"][i - 1] if i else None}[tail]
    if tail in ("mean", "var", "invstd"):
        return ops[tail][4 + i]
    if head == "dec4":
        return {"recon": ops["recon"], "mse": ops["mse"], "dd": ops["dd"][2]}[tail]
    return {"zd": ops["zd"][i], "d": ops["d"][i], "dzd": ops["dzd"][i], "dx": ops["de"][3] if i == 0 else ops["dd"][i - 1]}[tail]


# --------------------------------------------------------------------------------------------------------------- the comparator
UNEQUAL_CAP = 1e-3        # share of a case's bf16 elements (all stages pooled: the smallest tensors have 256) not bit-equal to bf16(want)
AMBIGUOUS_CAP = 1e-4      # share of a tensor's ReLU decisions that fp32 rounding leaves open
FP32_TOL, FLOOR_FACTOR = 1e-5, 8.0

# acc: the largest share of an element's accumulation allowance K u A that is in use once half a bf16 step (and any slack) is taken off
Row = namedtuple("Row", "name kind worst bound unequal ambiguous l2 l2_bound floor numel acc", defaults=(0, 0.0))


def _dev(got, want, scale, slack):
    """(max (|got - want| - slack) / scale, (||got - want|| - ||slack||) / ||want||), both >= 0"""
    d = (got - want).abs()
    s = slack if slack is not None else torch.zeros_like(d)
    wn = max(float(want.norm()), 1e-300)
    return max(float(((d - s) / scale).max()), 0.0), max((float(d.norm()) - float(s.norm())) / wn, 0.0)


def compare_one(name, res, got, floor_out=None, cap=1.0):
    """One stage's stored tensor `got` against its float64 Result -> Row.  bf16: worst = max over elements of |got - want| divided
    by the element's allowance 2^-8 |want| + cap * K u A (+ slack; half a bf16 step is arithmetic, not a cap), bound 1; the unequal
    share against cap * UNEQUAL_CAP, the ambiguous share against AMBIGUOUS_CAP.  fp32: worst = max |got - want| / scale and relative L2 (less the slack) against cap * max(1e-5, 8 * floor), floor = the
    same two measures of the float32 evaluation `floor_out` of the stage."""
    want = res.out.to(F64)
    got = got.detach().cpu().to(F64).reshape(want.shape)
    assert bool(torch.isfinite(got).all()), (name, "not finite")
    if res.kind == "bf16":
        allow = HALF_BF16 * want.abs() + cap * res.K * U * res.A
        if res.slack is not None:
            allow = allow + res.slack
        ratio = (got - want).abs() / allow.clamp_min(1e-300)
        ratio = torch.where((got - want).abs() == 0, torch.zeros_like(ratio), ratio)
        kua = (res.K * U * res.A).clamp_min(1e-300)
        acc = ((got - want).abs() - (allow - cap * res.K * U * res.A)).clamp_min(0) / kua
        amb_share = 0.0
        if res.amb is not None:
            alt_ratio = (got - res.alt.to(F64)).abs() / (HALF_BF16 * res.alt.abs() + cap * res.K * U * res.A).clamp_min(1e-300)
            ratio = torch.where(res.amb, torch.minimum(ratio, alt_ratio), ratio)
            acc = torch.where(res.amb, torch.minimum(acc, ((got - res.alt.to(F64)).abs() - HALF_BF16 * res.alt.abs()).clamp_min(0) / kua), acc)
            amb_share = float(res.amb.double().mean())
        unequal = bf16(want) != got
        if res.amb is not None:
            unequal &= ~(res.amb & (bf16(res.alt.to(F64)) == got))
        return Row(name, "bf16", float(ratio.max()), 1.0, float(unequal.double().mean()), amb_share, 0.0, 0.0, 0.0, unequal.numel(), float(acc.max()))
    if res.kind == "allow":     # a derived per-element allowance (res.slack) and nothing else: no floor, no tolerance on top
        ratio = (got - want).abs() / res.slack.to(F64).reshape(want.shape).clamp_min(1e-300)
        ratio = torch.where((got - want).abs() == 0, torch.zeros_like(ratio), ratio)
        return Row(name, "allow", float(ratio.max()), cap, 0.0, 0.0, 0.0, 0.0, 0.0, ratio.numel())
    scale = res.scale if res.scale is not None else max(float(want.abs().max()), 1e-300)
    emax, el2 = _dev(got, want, scale, res.slack)
    fmax = fl2 = 0.0
    if floor_out is not None:
        fmax, fl2 = _dev(floor_out.to(F64).reshape(want.shape), want, scale, None)
    if res.scale is not None:        # a sum that cancels: the L2 measure is taken against the same scale
        el2, fl2 = emax, fmax
    return Row(name, "fp32", emax, cap * max(FP32_TOL, FLOOR_FACTOR * fmax), 0.0, 0.0, el2, cap * max(FP32_TOL, FLOOR_FACTOR * fl2), fmax)


def unequal_share(rows):
    """the share of all bf16 elements of a case that are not bit-equal to bf16(want)"""
    n = sum(r.numel for r in rows if r.kind == "bf16")
    return sum(r.unequal * r.numel for r in rows if r.kind == "bf16") / max(n, 1)


def row_failures(row, cap=1.0):
    """what one stage misses (the unequal share is a criterion of the whole case: `compare`)"""
    bad = []
    if not row.worst <= row.bound:
        bad.append(f"{row.name}: {'max/scale' if row.kind == 'fp32' else 'element allowance ratio'} {row.worst:.3e} > {row.bound:.3e}"
                   + (f" (floor {row.floor:.2e})" if row.kind == "fp32" else ""))
    if not row.l2 <= row.l2_bound:
        bad.append(f"{row.name}: relative L2 {row.l2:.3e} > {row.l2_bound:.3e}")
    if not row.ambiguous <= AMBIGUOUS_CAP:
        bad.append(f"{row.name}: {row.ambiguous:.3e} of the ReLU decisions are open, cap {AMBIGUOUS_CAP:.1e}")
    return bad


def compare(want, got_of, floor=None, cap=1.0):
    """Every stage of `want` (stage_results in float64) whose stored tensor got_of(name) exists -> (rows, failures, names read)"""
    rows, bad, read = [], [], []
    for name, res in want.items():
        if res.kind == "share":
            rows.append(Row(name, "share", 0.0, 1.0, 0.0, float(res.out), 0.0, 0.0, 0.0))
            bad += row_failures(rows[-1], cap)
            continue
        got = got_of(name)
        if got is None:
            continue
        read.append(name)
        rows.append(compare_one(name, res, got, None if floor is None or res.kind != "fp32" else floor[name].out, cap))
        bad += row_failures(rows[-1], cap)
    if not unequal_share(rows) <= cap * UNEQUAL_CAP:
        bad.append(f"{unequal_share(rows):.3e} of the case's bf16 elements differ from bf16(want), cap {cap * UNEQUAL_CAP:.3e}")
    return rows, bad, read


def print_rows(tag, rows):
    """per case: the bf16 stage and the fp32 stage closest to their bounds, the largest unequal and ambiguous shares"""
    b = [r for r in rows if r.kind == "bf16"]
    f = [r for r in rows if r.kind == "fp32"]
    msg = f"[{tag}]"
    if b:
        w = max(b, key=lambda r: r.worst)
        u = max(b, key=lambda r: r.unequal)
        c = max(b, key=lambda r: r.acc)
        msg += f" bf16 worst {w.name}: {w.worst:.2f} of its allowance ({c.name}: {c.acc:.2f} of K u A beyond half a step); unequal {unequal_share(rows):.1e} of all (most: {u.name} {u.unequal:.1e})"
    if f:
        w = max(f, key=lambda r: max(r.worst / r.bound, r.l2 / r.l2_bound))
        msg += f"; fp32 worst {w.name}: max {w.worst:.1e} (floor {w.floor:.1e}, bound {w.bound:.1e}), l2 {w.l2:.1e} (bound {w.l2_bound:.1e})"
    a = max(rows, key=lambda r: r.ambiguous)
    msg += f"; open ReLU decisions {a.name} {a.ambiguous:.1e}"
    print(msg)
