"""tests/cnn1d_stage_oracle.py, dfa_cnn1d_train_plan and the criteria of tests/test_cnn1d_train_stages_gpu.py, pinned without a GPU.

  restatement   the stages chained in float64 with no rounding reproduce logits, loss, all 14 gradients and the batch statistics
                of tests/ragged_train_oracle.py::cnn1d_ragged_train_step (autograd over the definition of a ragged batch) to 1e-12
                of scale, at ragged sets and, with every length equal to T, at uniform shapes: both sides are float64, only the
                order of the sums differs.  oracle/torch_ref.py::cnn1d_train_step (the uniform oracle of
                tests/test_train_shapes_gpu.py) RETURNS float32, so it is met to 2^-22 of scale (its own rounding, twice), T = 2
                included, which the ragged oracle does not take.  The three convolution biases in front of a BatchNorm have
                gradient zero: both sides' rounding noise is held to the same share of the matching weight gradient's scale.
  floor         for every case, ragged set and dropout run of the GPU file, the float32 CPU evaluation of every stage, on operands
                made by the float64 chain with the fp32 roundings on, lies within 1e-5 of scale in both measures with no floor
                given (the 1e-5 term is no tighter than float32 arithmetic), and within 1.25e-6, an eighth of it, for every stage
                but the four of LOUD, whose float32 evaluation is noisier than that for a stated reason: there 8 floor, not
                1e-5, is the GPU file's bound.  (An eighth of max(1e-5, 8 floor) is met by the floor itself by construction
                wherever the floor exceeds 1.25e-6; it is evaluated too, and decides nothing for those four.)
  plan          dfa_cnn1d_train_plan with a NULL context: total, disjoint aligned ordered regions, the table of a ragged batch,
                cap, refusals.
  planted       eight faults the whole-step tests cannot see, each made by running the stage itself on the faulty operands or
                parameters, each rejected by the stage that reads it while its neighbours pass.
"""
import ctypes as C
import json
import os

import pytest
import torch

import cnn1d_stage_oracle as S
import ragged_train_oracle as RO
from oracle import torch_ref as R

SEED = 7
# stages whose CPU float32 evaluation exceeds 1.25e-6 of scale at some case (measured: up to 3.8e-6, 1.4e-6, 1.6e-6, 1.5e-6):
# dlogits = sigmoid(z) - y' and the loss cancel in float32 and at B = 1 are measured against a single value; the two wide weight
# gradients sum 642 products per element in float32 at [2,321,180]
LOUD = {"bce.dlogits", "bce.loss", "conv.4.weight", "conv.8.weight"}
_cache = {}


def _shape(case):
    """a uniform (B, T, F) or the name of a ragged set -> (B, T, F, lengths or None)"""
    if isinstance(case, str):
        lengths, T, F = S.RAGGED[case]
        return len(lengths), T, F, lengths
    return (*case, None)


def staged(case, p=0.0):
    """(state, operands of the fp32-rounded float64 chain, float64 stage results, float32 stage results), once per process"""
    if (case, p) not in _cache:
        B, T, F, lengths = _shape(case)
        sd = S.ordinary_state(SEED, F)
        x, y = S.case_input(B, T, F, lengths)
        keeps = None
        if p > 0:
            g = torch.Generator().manual_seed(11)
            keeps = (torch.rand(B, 32, T, generator=g) >= p, torch.rand(B, 64, T, generator=g) >= p)
        ops = S.run_chain(sd, x, y, lengths, p=p, keeps=keeps)
        if p > 0:
            ops["det"] = S.read_keeps(ops, sd)[1]
        _cache[(case, p)] = (sd, ops, S.stage_results(ops, sd), S.stage_results(ops, sd, S.F32, mags=False))
    return _cache[(case, p)]


def _close(got, want, tol, scale=None):
    want = want.to(S.F64)
    scale = float(want.abs().max()) if scale is None else scale
    assert scale > 0
    err = float((got.reshape(want.shape) - want).abs().max())
    assert err <= tol * scale, (err, scale)


@pytest.mark.parametrize("case", ["A", "D", (2, 33, 36), (3, 65, 20), (70, 5, 20)], ids=str)
def test_chained_stages_restate_the_ragged_autograd_oracle(case):
    B, T, F, lengths = _shape(case)
    sd = S.ordinary_state(SEED, F)
    x, y = S.case_input(B, T, F, lengths)
    o = S.run_chain(sd, x, y, lengths, fp32_points=False)
    w = RO.cnn1d_ragged_train_step(sd, torch.nan_to_num(x).transpose(1, 2), lengths or [T] * B, y, S.SMOOTHING)
    _close(o["logits"], w["logits"], 1e-12, max(1.0, float(w["logits"].abs().max())))
    assert abs(o["loss"] - w["loss"]) <= 1e-12 * abs(w["loss"])
    for l, bn in enumerate(S.BNL):
        mean, var, n = w["stats"][bn]
        assert n == o["n"]
        _close(o["mean"][l], mean, 1e-12)
        _close(o["var"][l], var, 1e-12)
    assert set(w["grads"]) == set(S.PARAM_ORDER) == set(o["grads"])
    noise = {c + ".bias": c + ".weight" for c in S.CONV}
    for name in S.PARAM_ORDER:
        _close(o["grads"][name], w["grads"][name], 1e-12, float(w["grads"][noise.get(name, name)].abs().max()))


@pytest.mark.parametrize("shape", [(3, 2, 20), (2, 31, 31), (3, 65, 20)], ids=str)
def test_chained_stages_restate_the_uniform_autograd_oracle(shape):
    sd = S.ordinary_state(SEED, shape[2])
    x, y = S.case_input(*shape)
    o = S.run_chain(sd, x, y, fp32_points=False)
    logits, loss, grads, stats = R.cnn1d_train_step(sd, x.transpose(1, 2), y, S.SMOOTHING, return_stats=True)
    tol = 2.0 ** -22            # the oracle returns float32
    _close(o["logits"], logits, tol, max(1.0, float(logits.abs().max())))
    assert abs(o["loss"] - loss) <= 1e-12 * abs(loss)
    for l, bn in enumerate(S.BNL):
        mean, var, n = stats[bn]
        assert n == o["n"]
        _close(o["mean"][l], mean, tol)
        _close(o["var"][l], var, tol)
    noise = {c + ".bias": c + ".weight" for c in S.CONV}
    for name in S.PARAM_ORDER:
        _close(o["grads"][name], grads[name], tol, float(grads[noise.get(name, name)].abs().max()))


def _floor(case, p):
    sd, ops, want, got32 = staged(case, p)
    rows, bad, read = S.compare(want, lambda n: got32[n].out, floor=got32, cap=0.125)
    S.print_rows(f"cpu float32 {case} p={p}", rows)
    assert not bad, "\n".join(bad)
    assert set(read) == S.stage_names()                                             # every stage was compared
    rows, bad, _ = S.compare(want, lambda n: got32[n].out)                          # no floor: everything within 1e-5
    assert not bad, "\n".join(bad)
    loud = [(r.name, r.worst, r.l2) for r in rows if r.kind == "fp32" and r.name not in LOUD and max(r.worst, r.l2) > 1.25e-6]
    assert not loud, loud
    assert not S.padding_failures(ops)
    # the chain's own stored tensors are fp32(stage on its operands): the chain and stage_results state the same thing
    for name, res in want.items():
        if res.kind == "fp32" and name != "bce.loss" and not name.endswith("invstd") and name not in ops["grads"]:
            got = S.stored_of(ops, name)
            assert torch.equal(S.f32r(res.out).reshape(got.shape), got), name
    if p > 0:   # the keep masks are recovered from the stored tensors wherever they are determined
        keeps, det = S.read_keeps(ops, sd)
        for k, d, true in zip(keeps, det, ops["keep"]):
            assert torch.equal(k[d], true[d].bool()) and bool(k[~d].all()) and 0.2 < float(d.double().mean()) < 1.0
        assert not S.kept_share_failures(keeps, det, p)


@pytest.mark.parametrize("case", S.CASES + list(S.RAGGED), ids=str)
def test_float32_stages_lie_within_the_fp32_criterion(case):
    _floor(case, 0.0)


@pytest.mark.parametrize("case", [(2, 33, 36), (2, 321, 180), "A", "B"], ids=str)
def test_float32_stages_lie_within_the_fp32_criterion_with_dropout(case):
    _floor(case, 0.3)


def test_two_term_convolutions_get_their_derived_allowance_and_no_more():
    """conv_terms=2: a convolution whose operands are cut to two bf16 terms (the kept products of conv1d_x3_kernel<MT, 2>) passes;
    one cut to ONE term per operand does not"""
    sd, ops, _, _ = staged("A")
    want = S.stage_results(ops, sd, conv_terms=2)
    P = S._params(sd)

    def terms(t, n):
        hi = t.to(torch.float32).to(torch.bfloat16).to(S.F64)
        return (hi, (t - hi).to(torch.float32).to(torch.bfloat16).to(S.F64)) if n == 2 else (hi, torch.zeros_like(hi))
    w0, w1 = terms(P["conv.4.weight"], 2)
    a0, a1 = terms(ops["h"][0], 2)
    b, v = P["conv.4.bias"], ops["valid"]
    zero = torch.zeros_like(b)
    two = S.conv1d(a0, w0, b, v).out + S.conv1d(a1, w0, zero, v).out + S.conv1d(a0, w1, zero, v).out
    sel = v.expand(two.shape)
    assert not S.row_failures(S.compare_one("l2.z", want["l2.z"], two[sel]))
    assert float((two - S.conv1d(ops["h"][0], P["conv.4.weight"], b, v).out).abs().max()) > 0
    assert S.row_failures(S.compare_one("l2.z", want["l2.z"], S.conv1d(a0, w0, b, v).out[sel]))


def _reject(want, name, got, floor=None):
    return S.row_failures(S.compare_one(name, want[name], got, None if floor is None else floor[name].out))


def _with(ops, **kw):
    o = dict(ops)
    o.update(kw)
    return o


def test_planted_faults_are_rejected():
    """each fault is rejected by the stage that reads it; the float32 outputs of that stage and of its neighbours pass"""
    sd, ops, want, got32 = staged("A", 0.3)
    P = S._params(sd)
    lengths, T_max, _ = S.RAGGED["A"]
    B, v, n = len(lengths), ops["valid"], ops["n"]
    sel = {c: v.expand(-1, c, -1) for c in S.BN_C}
    for name in S.stage_names():
        assert not _reject(want, name, got32[name].out, got32), name                   # the unbroken outputs pass
    # 1. layer 2's keep mask regenerated for layer 1's backward (dc.layer), 2. the keep-scale left out of the backward
    wrong_mask = _with(ops, keep=[ops["keep"][1][:, :32], ops["keep"][1]])
    no_scale = _with(ops, keep=[ops["keep"][0] / S.keep_scale(0.3), ops["keep"][1]])
    for what, o in (("layer 2's keep mask in layer 1's backward", wrong_mask), ("no keep-scale in the backward", no_scale)):
        bad = S.stage_results(o, sd, mags=False)
        for name in ("l1.dz", "conv.1.weight", "conv.1.bias"):
            assert _reject(want, name, bad[name].out, got32), f"{what}: {name} was accepted"
    # 3. the time mean divided by T_max
    got = S.time_mean(ops["z"][2], *S._bnp(ops, P, 2), torch.full((B,), float(T_max), dtype=S.F64), v)[0]
    assert _reject(want, "pooled", got, got32)
    # (the bound of pooled is the fp32 criterion plus the open decisions' magnitude only: 1.5e-5 of scale on one element fails
    # at the smallest case, where a K u A allowance over every frame would have doubled the bound)
    _, _, w3, f3 = staged((1, 3, 20))
    off = f3["pooled"].out.to(S.F64).clone()
    off[0, 0] += 1.5e-5 * float(w3["pooled"].out.abs().max())
    assert _reject(w3, "pooled", off, f3) and not _reject(w3, "pooled", f3["pooled"].out, f3)
    # 4. the statistics over all B T_max frames: the stage run on the whole padded tensor
    for l in (1, 2, 3):
        m, var = S.batch_stats(S._cl(ops["z"][l - 1]))
        assert _reject(want, f"l{l}.mean", m, got32) and _reject(want, f"l{l}.var", var, got32)
        assert _reject(want, f"l{l}.running_var", S.MOMENTUM * var * (B * T_max) / (B * T_max - 1)
                       + (1 - S.MOMENTUM) * P[S.BNL[l - 1] + ".running_var"], got32)
    # 5. an unflipped data-gradient tap
    for l in (1, 2):
        got = S.conv1d_dgrad(ops["dz"][l], P[S.CONV[l] + ".weight"].flip(2), v).out
        assert _reject(want, f"l{l + 1}.dx", got[sel[S.BN_C[l - 1]]], got32)
    # 6. a tap reaching across an utterance's last frame: the frame behind it is not read as zero
    h1 = ops["h"][0].clone()
    for b, t in enumerate(lengths):
        if t < T_max:
            h1[b, :, t] = h1[b, :, t - 1]
    got = S.conv1d(h1, P["conv.4.weight"], P["conv.4.bias"], torch.ones_like(v)).out
    assert _reject(want, "l2.z", got[sel[64]], got32)
    got = S.conv1d_wgrad(ops["dz"][1], h1, torch.ones_like(v))[0]
    assert _reject(want, "conv.4.weight", got, got32), "tap 2 of the weight gradient reads h1 behind the last frame"
    assert S.padding_failures(_with(ops, h=[h1, ops["h"][1]]))
    dz2 = ops["dz"][1].clone()
    for b, t in enumerate(lengths):
        if t < T_max:
            dz2[b, :, t] = dz2[b, :, t - 1]
    assert _reject(want, "conv.4.weight", S.conv1d_wgrad(dz2, ops["h"][0], torch.ones_like(v))[0], got32)
    assert S.padding_failures(_with(ops, dz=[ops["dz"][0], dz2, ops["dz"][2]]))
    # 7. the weight gradient on the un-rolled x (a uniform batch under a time roll)
    sdu = S.ordinary_state(SEED, 36)
    x, y = S.case_input(2, 33, 36)
    ou = S.run_chain(sdu, torch.roll(x, 3, dims=2), y)
    wu, fu = S.stage_results(ou, sdu), S.stage_results(ou, sdu, S.F32, mags=False)
    assert _reject(wu, "conv.0.weight", S.conv1d_wgrad(ou["dz"][0], x, ou["valid"])[0], fu)
    assert not _reject(wu, "conv.0.weight", fu["conv.0.weight"].out, fu) and not _reject(wu, "conv.0.bias", fu["conv.0.bias"].out, fu)
    # 8. one empty batch chunk's record left non-zero: a stale record (utterance 0's own) enters the reduction once more -- the
    # reductions run on the batch with utterance 0 appended again
    sdd, od, wd, fd = staged((70, 5, 20))
    Pd = S._params(sdd)
    again = lambda t: torch.cat([t, t[:1]])      # noqa: E731
    vd = again(od["valid"])
    up = S.upstream(od, 1, od["valid"])
    red = S.bn_bwd_reduce(S._cl(again(od["z"][1])), S._cl(again(up)), *S._bnp(od, Pd, 1))
    assert _reject(wd, "conv.5.bias", red.S1, fd) and _reject(wd, "conv.5.weight", red.S2, fd)
    dW, db = S.conv1d_wgrad(again(od["dz"][1]), again(od["h"][0]), vd)
    assert _reject(wd, "conv.4.weight", dW, fd) and _reject(wd, "conv.4.bias", db, fd)
    for name in ("conv.5.bias", "conv.5.weight", "conv.4.weight", "conv.4.bias", "l2.dz", "l2.z"):
        assert not _reject(wd, name, fd[name].out, fd), name


# ------------------------------------------------------------------------------------------------------------------ the plan
@pytest.mark.parametrize("ragged", [False, True], ids=["uniform", "ragged"])
def test_train_plan_reports_distinct_ordered_regions(ragged):
    from dfa_amd import _lib
    lib = _lib.load()
    shapes = [s for s in S.CASES if s[1] >= 3 or not ragged] + [(len(l), t, f) for l, t, f in S.RAGGED.values()] + [(256, 321, 180)]
    for B, T, F in shapes:
        pl = _lib.cnn1d_train_plan(None, B, T, F, ragged)
        nbytes = lib.dfa_cnn1d_train_ragged_workspace_bytes if ragged else lib.dfa_cnn1d_train_workspace_bytes
        assert pl.total == nbytes(None, B, T, F) > 0
        regions = [(f"{k}{l}", getattr(pl, k)[l], B * c * T * 4) for k, cs in (("z", S.BN_C), ("h", S.BN_C[:2])) for l, c in enumerate(cs)]
        regions += [("pooled", pl.pooled, B * 128 * 4), ("dpooled", pl.dpooled, B * 128 * 4)]
        regions += [(f"{k}{l}", getattr(pl, k)[l], B * c * T * 4) for k, cs in (("dz", S.BN_C), ("dh", S.BN_C[:2])) for l, c in enumerate(cs)]
        regions += [("stats", pl.stats, 3 * sum(S.BN_C) * 4), ("sums", pl.sums, 2 * sum(S.BN_C) * 4), ("partial", pl.partial, pl.partial_bytes)]
        if ragged:
            regions.append(("lengths", pl.lengths, 2 * B * 4))
            assert pl.lengths == lib.dfa_cnn1d_train_workspace_bytes(None, B, T, F)
        else:
            assert pl.lengths == -1
        assert [r[1] for r in regions] == list(pl.fields[:15]) + ([pl.lengths] if ragged else []) and regions[0][1] == 0
        for (a, off, size), (_, nxt, _) in zip(regions, regions[1:] + [("total", pl.total, 0)]):
            assert off % 256 == 0 and 0 <= nxt - off - size < 256, (a, "overlap or more than alignment padding", (B, T, F))
        # the reductions' records fit: 64 (256) batch chunks of the channel-major (weight-gradient) kernels
        assert pl.partial_bytes >= max(min(B, 64) * 128 * 2 * 4, min(B, 256) * (128 * 64 * 3 + 128) * 4, min(B, 256) * (32 * F * 3 + 32) * 4)
    # cap: only the first `cap` fields are written, the count is returned all the same; NULL only validates
    n = _lib.Cnn1dTrainPlan.NFIELDS
    buf = (C.c_longlong * n)(*([-7] * n))
    assert lib.dfa_cnn1d_train_plan(None, 2, 33, 36, int(ragged), buf, 3) == n == lib.dfa_cnn1d_train_plan(None, 2, 33, 36, int(ragged), None, 0)
    assert list(buf)[:3] == list(_lib.cnn1d_train_plan(None, 2, 33, 36, ragged).z) and set(list(buf)[3:]) == {-7}
    refused = [(0, 8, 20), (2, 0, 20), (2, 8, 0)] + ([(2, 2, 20)] if ragged else [])
    for shape in refused:
        assert lib.dfa_cnn1d_train_plan(None, *shape, int(ragged), None, 0) == _lib.E_BAD_SHAPE
        with pytest.raises(ValueError):
            _lib.cnn1d_train_plan(None, *shape, ragged)
    if not ragged:
        assert lib.dfa_cnn1d_train_plan(None, 3, 2, 20, 0, None, 0) == n               # T = 2 is a uniform shape
    # the codes are the golden ones of the step (the messages need a context: tests/test_cnn1d_train_stages_gpu.py)
    golden = {name: code for name, code, _ in json.load(open(os.path.join(os.path.dirname(__file__), "golden", "abi_train_errors.json")))}
    pre = "cnn1d_forward_train_ragged/" if ragged else "cnn1d_forward_train/"
    assert golden[pre + "batch_0"] == golden[pre + "T_0"] == golden["cnn1d_train_plan/F_0"] == _lib.E_BAD_SHAPE
    assert golden["cnn1d_forward_train_ragged/T_short"] == _lib.E_BAD_SHAPE
