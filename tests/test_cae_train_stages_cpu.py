"""tests/cae_stage_oracle.py and the criteria of tests/test_cae_train_stages_gpu.py, pinned without a GPU.

  restatement   the stages chained in float64 with every rounding off reproduce the loss and all 30 gradients of
                oracle/torch_ref.py::cae_train_step_emulated(emulate=None) to 1e-9 of scale (both sides float64; only the order
                of the sums differs).  The seven convolution biases in front of a BatchNorm have gradient zero: both sides'
                rounding noise is held to 1e-9 of the matching weight gradient's scale.
  caps          for every case of the GPU file, the float32 CPU evaluation of every stage, on operands made by the float64 chain
                with the bf16 roundings on, meets the GPU file's criteria with an eighth of each cap: the fp32 accumulation
                allowance K u A / 8 beside half a bf16 step, at most 1.25e-4 of a tensor's elements not bit-equal to
                bf16(float64), at most 1e-4 of a tensor's ReLU decisions open.  So the caps are the reference arithmetic's own
                error with room, never the code's under test.
  planted       a correct stage output broken the way strip kernels break is rejected by the same comparator, at the smallest and
                the largest case.
"""
import pytest
import torch

import cae_stage_oracle as S
from oracle import torch_ref as R

SEED = 7
_cache = {}


def staged(shape):
    """(state, operands of the rounded float64 chain, float64 stage results, float32 stage results), once per process"""
    if shape not in _cache:
        sd = S.ordinary_state(SEED)
        ops = S.run_chain(sd, S.case_input(*shape))
        _cache[shape] = (sd, ops, S.stage_results(ops, sd), S.stage_results(ops, sd, S.F32, full=False))
    return _cache[shape]


@pytest.mark.parametrize("shape", [(2, 17, 20), (3, 31, 36), (2, 47, 52)], ids=str)
def test_chained_stages_restate_the_autograd_oracle(shape):
    sd, x = S.ordinary_state(SEED), S.case_input(*shape)
    o = S.run_chain(sd, x, rounding=False)
    loss, grads = R.cae_train_step_emulated(sd, x, emulate=None, unrounded_grads=True)
    assert abs(o["loss"] - loss) <= 1e-9 * abs(loss)
    assert set(grads) == set(S.PARAM_ORDER) == set(o["grads"])
    noise = {f"{seq}.{c}.bias": f"{seq}.{c}.weight" for seq, idx in (("encoder", S.ENC_IDX), ("decoder", S.DEC_IDX)) for c, _ in idx}
    for name in S.PARAM_ORDER:
        want = grads[name].to(S.F64)
        got = o["grads"][name].reshape(want.shape)
        scale = float(grads[noise.get(name, name)].abs().max())
        assert scale > 0
        assert float((got - want).abs().max()) <= 1e-9 * scale, (name, float((got - want).abs().max()), scale)


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_train_plan_reports_distinct_regions(prec):
    """dfa_cae_train_plan: the dimensions follow the model, the total is the byte planner's, and the regions the stage tests read
    (every stored tensor and the statistics block) are disjoint and inside the workspace; refusals carry the step's own codes."""
    from dfa_amd import _lib
    lib, code = _lib.load(), _lib.PRECISIONS[prec]
    for B, T, F in S.CASES + [(5, 64, 36), (1, 4001, 180)]:
        pl = _lib.cae_train_plan(None, B, T, F, code)
        assert pl.total == lib.dfa_cae_train_workspace_bytes(None, B, T, F, code) and pl.elem == (2 if prec == "bf16" else 4)
        assert pl.H == (T, T // 2, T // 4, T // 8, T // 16) and pl.W == (F, F // 2, F // 4, F // 8, F // 16)
        assert pl.Hd == tuple((T // 16) * 2 ** k for k in (1, 2, 3, 4)) and pl.Wd[3] == F and pl.Wd[1] == 2 * pl.Wd[0] + 1
        assert pl.C == S.ENC_C + S.DEC_C and pl.z[0] == -1 and pl.dz[0] == -1
        spans = [(pl.stats, 3 * sum(pl.C) * 4, "stats")]
        for key, dims in (("e", [(pl.H[l + 1], pl.W[l + 1], pl.C[l]) for l in range(4)]),
                          ("de", [(pl.H[l + 1], pl.W[l + 1], pl.C[l]) for l in range(4)]),
                          ("z", [(pl.H[l], pl.W[l], pl.C[l]) for l in range(4)]), ("dz", [(pl.H[l], pl.W[l], pl.C[l]) for l in range(4)]),
                          *((k, [(pl.Hd[l], pl.Wd[l], pl.C[4 + l]) for l in range(3)]) for k in ("zd", "d", "dd", "dzd"))):
            for l, (off, (H, W, C)) in enumerate(zip(getattr(pl, key), dims)):
                if off >= 0:
                    spans.append((off, B * H * W * C * pl.elem, f"{key}[{l}]"))
        for off, n, name in ((pl.zp, 1, "zp"), (pl.xf, 1, "xf"), (pl.wq, 256 * 512 * 4, "wq"), (pl.dwq, 256 * 512 * 4, "dwq"),
                             (pl.partial, pl.partial_bytes, "partial")):
            spans.append((off, n, name))
        spans.sort()
        for (o0, n0, a), (o1, _, b) in zip(spans, spans[1:]):
            assert o0 % 256 == 0 and o0 + n0 <= o1, (a, b, "overlap", (B, T, F))
        assert spans[-1][0] + spans[-1][1] <= pl.total
        for i in range(7):
            assert pl.stats <= pl.mean[i] < pl.var[i] < pl.invstd[i] and pl.var[i] - pl.mean[i] == 4 * pl.C[i] == pl.invstd[i] - pl.var[i]
            assert i == 6 or pl.invstd[i] + 4 * pl.C[i] == pl.mean[i + 1]
    for shape, err in (((0, 16, 20), _lib.E_BAD_SHAPE), ((1, 15, 20), _lib.E_BAD_SHAPE), ((1, 16, 32), _lib.E_BAD_SHAPE)):
        assert lib.dfa_cae_train_plan(None, *shape, code, None, 0) == err
        with pytest.raises(ValueError):
            _lib.cae_train_plan(None, *shape, code)
    assert lib.dfa_cae_train_plan(None, 1, 16, 20, 7, None, 0) == _lib.E_BAD_DTYPE


def _cpu_got(want, got32):
    def got_of(name):
        r = got32[name]
        return S.bf16(r.out) if want[name].kind == "bf16" else r.out
    return got_of


@pytest.mark.parametrize("shape", S.CASES, ids=str)
def test_float32_stages_meet_an_eighth_of_every_cap(shape):
    sd, ops, want, got32 = staged(shape)
    rows, bad, read = S.compare(want, _cpu_got(want, got32), floor=got32, cap=0.125)
    S.print_rows(f"cpu float32 {list(shape)}", rows)
    assert not bad, "\n".join(bad)
    assert len(read) == len([r for r in want.values() if r.kind != "share"])      # every stage was compared
    # the chain's own stored tensors are bf16(stage on its operands): the chain and stage_results state the same thing
    for name, res in want.items():
        if res.kind == "bf16":
            assert torch.equal(S.bf16(res.out), S.stored_of(ops, name)), name


def _reject(want, name, got, floor=None):
    row = S.compare_one(name, want[name], got, None if floor is None else floor[name].out)
    return S.row_failures(row)


@pytest.mark.parametrize("shape", [S.CASES[0], max(S.CASES, key=lambda s: s[0] * s[1] * s[2])], ids=str)
def test_planted_faults_are_rejected(shape):
    sd, ops, want, got32 = staged(shape)
    good = {n: S.bf16(r.out) for n, r in want.items() if r.kind == "bf16"}
    for name, g in good.items():
        assert not _reject(want, name, g), name                                 # the unbroken outputs pass
    P = S._params(sd)
    faults = []
    z = good["enc2.z"]                       # [B, H1, W1, 64]: the first strip-kernel output
    H, W = z.shape[1:3]
    t = z.clone(); t[:, -1] = 0
    faults.append(("last row zero", "enc2.z", t))
    dz = good["enc2.dz"]
    t = dz.clone(); t[:, 2 * (H // 2) - 1] = 0        # the last pooled row: the neighbour of the dropped one where H is odd
    faults.append(("dropped row's neighbour zero", "enc2.dz", t))
    dx = good["enc2.dx"]                     # the data gradient at the same height: every row receives gradient, the dropped one too
    t = dx.clone(); t[:, 2 * (H // 2) - 1] = 0
    faults.append(("dropped row's neighbour zero in the data gradient", "enc2.dx", t))
    t = z.clone(); w = min(32, W); t[:, :, :w] = torch.roll(z[:, :, :w], 1, dims=2)
    faults.append(("one 32-column strip shifted by a column", "enc2.z", t))
    t = z.clone(); t[..., 9], t[..., 10] = z[..., 10], z[..., 9]
    faults.append(("two channels of one group of 8 swapped", "enc2.z", t))
    d = good["dec2.d"]                       # BatchNorm + ReLU of the layer with the output_padding column
    t = d.clone(); t[:, :, -1, :] = S.bf16(P["decoder.3.bias"])
    faults.append(("output_padding column left at the bias", "dec2.d", t))
    zd = good["dec2.zd"]
    t = zd.clone(); t[:, :, -1, :] = zd[:, :, -2, :]
    faults.append(("output_padding column filled from its neighbour", "dec2.zd", t))
    for what, name, got in faults:
        assert _reject(want, name, got), f"{what}: {name} was accepted at {shape}"
    # one pixel missing from a weight-gradient sum (3x3 convolution and ConvTranspose2d) and from a bias-gradient sum
    dzs, e0 = ops["dz"][1], ops["e"][0]
    one = torch.zeros_like(dzs); one[0, H // 2, W // 2] = dzs[0, H // 2, W // 2]
    dW1, db1 = S.conv3x3_wgrad(one, e0)
    assert _reject(want, "encoder.4.weight", want["encoder.4.weight"].out - dW1, got32)
    assert _reject(want, "encoder.4.bias", want["encoder.4.bias"].out - db1, got32)
    dzd, src = ops["dzd"][1], ops["d"][0]
    one = torch.zeros_like(dzd); one[0, 1, 1] = dzd[0, 1, 1]
    dWt, _ = S.convt_wgrad(src, one)
    assert _reject(want, "decoder.3.weight", want["decoder.3.weight"].out - dWt, got32)
    # the bias gradient of the ConvTranspose2d must count the output_padding column
    col = dzd[:, :, -1, :].sum(dim=(0, 1))
    assert _reject(want, "decoder.3.bias", want["decoder.3.bias"].out - col, got32)
    # and the float32 stages themselves pass the fp32 criterion against their own floor
    for name in ("encoder.4.weight", "encoder.4.bias", "decoder.3.weight", "decoder.3.bias"):
        assert not _reject(want, name, got32[name].out, got32), name
