"""tests/cnn2d_stage_oracle.py, dfa_cnn2d_train_plan and the criteria of tests/test_cnn2d_train_stages_gpu.py, pinned without a GPU.

  restatement   the stages chained in float64 with every rounding off reproduce logits, loss, all 14 gradients and the batch
                statistics of oracle/torch_ref.py::cnn2d_train_step_emulated(emulate=None) (pinned to the reference's own autograd
                by tests/test_oracle_golden.py) to 1e-12 of scale: both sides are float64, only the order of the sums differs.
                With the bf16 roundings on they reproduce emulate="bf16" to 1e-9 of scale -- the same stored values bit for bit,
                so again only summation order remains -- once the S2 term of dz takes xhat from the unrounded accumulators as
                torch autograd does there (run_chain's autograd_xhat; the kernels take the stored z, which is what the stages
                state).  The three convolution biases in front of a BatchNorm have gradient zero: both sides' rounding noise is
                held to the same share of the matching weight gradient's scale.
  caps          for every case of the GPU file, the float32 CPU evaluation of every stage, on operands made by the float64 chain
                with the roundings on, meets the GPU file's criteria with an eighth of each cap (with and without dropout).
  plan          dfa_cnn2d_train_plan with a NULL context: dimensions, total, disjoint aligned ordered regions, cap, refusals.
"""
import ctypes as C
import json
import os

import pytest
import torch

import cnn2d_stage_oracle as S
from oracle import torch_ref as R

SEED = 7
_cache = {}


def staged(shape, p=0.0):
    """(state, operands of the rounded float64 chain, float64 stage results, float32 stage results), once per process"""
    if (shape, p) not in _cache:
        B, T, F = shape
        sd = S.ordinary_state(SEED, F)
        x, y = S.case_input(*shape)
        keeps = None
        if p > 0:
            g = torch.Generator().manual_seed(11)
            keeps = (torch.rand(B, T // 2, F, 32, generator=g) >= p, torch.rand(B, T // 4, F, 64, generator=g) >= p)
        ops = S.run_chain(sd, x, y, p=p, keeps=keeps)
        _cache[(shape, p)] = (sd, ops, S.stage_results(ops, sd), S.stage_results(ops, sd, S.F32, mags=False))
    return _cache[(shape, p)]


@pytest.mark.parametrize("emulate", [None, "bf16"])
@pytest.mark.parametrize("shape", [(2, 7, 31), (3, 21, 65)], ids=str)
def test_chained_stages_restate_the_autograd_oracle(shape, emulate):
    sd = S.ordinary_state(SEED, shape[2])
    x, y = S.case_input(*shape)
    on = emulate == "bf16"
    tol = 1e-9 if on else 1e-12
    o = S.run_chain(sd, x, y, rounding=on, fp32_points=False, autograd_xhat=on)
    logits, loss, grads, stats = R.cnn2d_train_step_emulated(sd, x, y, S.SMOOTHING, emulate, return_stats=True, unrounded=True)
    assert float((o["logits"] - logits).abs().max()) <= tol * max(1.0, float(logits.abs().max()))
    assert abs(o["loss"] - loss) <= tol * abs(loss)
    for l, bn in enumerate(S.BNL):
        mean, var, n = stats[bn]
        assert n == o["n"][l]
        assert float((o["mean"][l] - mean).abs().max()) <= tol * float(mean.abs().max())
        assert float((o["var"][l] - var).abs().max()) <= tol * float(var.abs().max())
    assert set(grads) == set(S.PARAM_ORDER) == set(o["grads"])
    noise = {c + ".bias": c + ".weight" for c in S.CONV}
    for name in S.PARAM_ORDER:
        want = grads[name].to(S.F64)
        got = o["grads"][name].reshape(want.shape)
        scale = float(grads[noise.get(name, name)].abs().max())
        assert scale > 0
        assert float((got - want).abs().max()) <= tol * scale, (name, float((got - want).abs().max()), scale)


def _cpu_got(want, got32):
    def got_of(name):
        r = got32[name]
        return S.bf16(r.out) if want[name].kind == "bf16" else r.out
    return got_of


@pytest.mark.parametrize("shape", S.CASES, ids=str)
def test_float32_stages_meet_an_eighth_of_every_cap(shape):
    _eighth(shape, 0.0)


@pytest.mark.parametrize("shape", [(2, 7, 31), (3, 21, 65), (2, 321, 180)], ids=str)
def test_float32_stages_meet_an_eighth_of_every_cap_with_dropout(shape):
    _eighth(shape, 0.3)


def _eighth(shape, p):
    sd, ops, want, got32 = staged(shape, p)
    rows, bad, read = S.compare(want, _cpu_got(want, got32), floor=got32, cap=0.125)
    S.print_rows(f"cpu float32 {list(shape)} p={p}", rows)
    assert not bad, "\n".join(bad)
    assert len(read) == len([r for r in want.values() if r.kind != "share"])      # every stage was compared
    # the chain's own stored tensors are bf16(stage on its operands): the chain and stage_results state the same thing
    for name, res in want.items():
        if res.kind == "bf16":
            assert torch.equal(S.bf16(res.out), S.stored_of(ops, name)), name
    if p > 0:   # the keep masks are recovered from the stored tensors wherever they are determined
        keeps, det = S.read_keeps(ops, sd, p)
        for k, d, true in zip(keeps, det, ops["keep"]):
            assert torch.equal(k[d], true[d].bool()) and bool(k[~d].all()) and 0.5 < float(d.double().mean()) < 1.0


def test_float32_stages_in_fp32_storage_meet_an_eighth_of_every_cap():
    """the fp32-precision statement (unrounded weights, every stored tensor under the fp32 criterion) on unrounded operands"""
    shape = (2, 7, 31)
    sd = S.ordinary_state(SEED, shape[2])
    ops = S.run_chain(sd, *S.case_input(*shape), rounding=False, fp32_points=True)
    want = S.stage_results(ops, sd, elem="fp32")
    got32 = S.stage_results(ops, sd, S.F32, mags=False, elem="fp32")
    rows, bad, read = S.compare(want, lambda n: got32[n].out, floor=got32, cap=0.125)
    assert not bad, "\n".join(bad)
    assert not [r for r in rows if r.kind == "bf16"]


def _reject(want, name, got, floor=None):
    return S.row_failures(S.compare_one(name, want[name], got, None if floor is None else floor[name].out))


@pytest.mark.parametrize("shape", [(2, 7, 31), (2, 321, 180)], ids=str)
def test_planted_faults_are_rejected(shape):
    """a correct stage output broken the way strip kernels, pools and reductions break is rejected by the comparator"""
    sd, ops, want, got32 = staged(shape)
    good = {n: S.bf16(r.out) for n, r in want.items() if r.kind == "bf16"}
    for name, g in good.items():
        assert not _reject(want, name, g), name                                 # the unbroken outputs pass
    faults = []
    for name in ("b2.z", "b3.z"):            # the two strip kernels' outputs
        z = good[name]
        W = z.shape[2]
        t = z.clone(); t[:, :, -1] = 0
        faults.append(("last strip column zero", name, t))
        t = z.clone(); w = min(30, W); t[:, :, :w] = torch.roll(z[:, :, :w], 1, dims=2)
        faults.append(("one strip shifted by a column", name, t))
        t = z.clone(); t[..., 9], t[..., 10] = z[..., 10], z[..., 9]
        faults.append(("two channels of one group of 8 swapped", name, t))
    for name in ("b2.dz", "b3.dx", "b2.dx", "b1.a", "b2.a"):
        t = good[name].clone(); t[:, -1] = 0
        faults.append(("last row zero (the dropped row's dz2 where H1 is odd)", name, t))
    t = good["b2.a"].clone(); t[:, -1] = 2 * t[:, -1]
    faults.append(("the last pooled row a sum, not a mean", "b2.a", t))
    for what, name, got in faults:
        assert _reject(want, name, got), f"{what}: {name} was accepted at {shape}"
    # fp32 outputs: one pixel missing from a weight-gradient sum, one frame from the time mean, one count of msum, the dropped row
    # missing from block 1's statistics
    dz, a1 = ops["dz2"], ops["a1"]
    one = torch.zeros_like(dz); one[0, 0, 0] = dz[0, 0, 0]
    assert _reject(want, "conv.5.weight", want["conv.5.weight"].out - S.conv3x3_wgrad(one, a1)[0], got32)
    H2 = ops["z3"].shape[1]
    if H2 > 1:
        emb1 = S.time_mean(ops["z3"][:, :-1], *S._bnp(ops, S._params(sd), 2))[0] * (H2 - 1) / H2
        assert _reject(want, "b3.emb", emb1, got32)
    n = want["b3.msum.n"].out.clone(); n[0, 0, 0] += 1
    assert _reject(want, "b3.msum.n", n, got32)
    if shape[1] % 2:
        P = S._params(sd)
        m = S.batch_stats(S.conv3x3(ops["x"][:, :-1].unsqueeze(-1), P["conv.0.weight"], P["conv.0.bias"]).out)[0]
        assert _reject(want, "b1.mean", m, got32)
    for name in ("conv.5.weight", "b3.emb", "b3.msum.n", "b1.mean"):
        assert not _reject(want, name, got32[name].out, got32), name


# ------------------------------------------------------------------------------------------------------------------ the plan
ACT = {"a1": ("H1", 32), "z2": ("H1", 64), "a2": ("H2", 64), "z3": ("H2", 128), "dz3": ("H2", 128), "da2": ("H2", 64), "dz2": ("H1", 64),
       "da1": ("H1", 32)}


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_train_plan_reports_distinct_ordered_regions(prec):
    from dfa_amd import _lib
    lib, code = _lib.load(), _lib.PRECISIONS[prec]
    for B, T, F in S.CASES + [(5, 64, 36), (256, 321, 180)]:
        pl = _lib.cnn2d_train_plan(None, B, T, F, code)
        assert pl.total == lib.dfa_cnn2d_train_workspace_bytes(None, B, T, F, code) and pl.elem == (2 if prec == "bf16" else 4)
        assert (pl.H1, pl.H2) == (T // 2, T // 4)
        size = {k: B * getattr(pl, h) * F * c * pl.elem for k, (h, c) in ACT.items()}
        size.update(emb=B * 128 * F * 4, demb=B * 128 * F * 4, msum=B * 128 * F * 2 * 4, raw=B * pl.H2 * F * 64 * 4, stats=3 * sum(S.BN_C) * 4,
                    sums=(2 * sum(S.BN_C) + 32 * 11 + 90) * 4, partial=pl.partial_bytes)
        order = [n for n in _lib.CNN2D_TRAIN_PLAN_FIELDS if n in size]
        assert order == list(_lib.CNN2D_TRAIN_PLAN_FIELDS[3:18]) and getattr(pl, order[0]) == 0
        for a, b in zip(order, order[1:] + ["total"]):
            assert getattr(pl, a) % 256 == 0 and getattr(pl, a) + size[a] <= getattr(pl, b), (a, b, (B, T, F))
            assert getattr(pl, b) - getattr(pl, a) - size[a] < 256 or a in ("sums",), (a, "more than alignment padding", (B, T, F))
    # cap: only the first `cap` fields are written, the count is returned all the same; NULL only validates
    n = len(_lib.CNN2D_TRAIN_PLAN_FIELDS)
    buf = (C.c_longlong * n)(*([-7] * n))
    assert lib.dfa_cnn2d_train_plan(None, 2, 7, 31, code, buf, 3) == n == lib.dfa_cnn2d_train_plan(None, 2, 7, 31, code, None, 0)
    assert list(buf)[:3] == [3, 1, 2 if prec == "bf16" else 4] and set(list(buf)[3:]) == {-7}
    for shape, err in (((0, 8, 20), _lib.E_BAD_SHAPE), ((2, 3, 20), _lib.E_BAD_SHAPE), ((2, 8, 0), _lib.E_BAD_SHAPE)):
        assert lib.dfa_cnn2d_train_plan(None, *shape, code, None, 0) == err
        with pytest.raises(ValueError):
            _lib.cnn2d_train_plan(None, *shape, code)
    assert lib.dfa_cnn2d_train_plan(None, 2, 8, 20, 3, None, 0) == _lib.E_BAD_DTYPE
    # the codes are the golden ones of the step (the messages need a context: tests/test_cnn2d_train_stages_gpu.py)
    golden = {name: code_ for name, code_, _ in json.load(open(os.path.join(os.path.dirname(__file__), "golden", "abi_train_errors.json")))}
    assert golden["cnn2d_forward_train/precision"] == _lib.E_BAD_DTYPE
    assert golden["cnn2d_forward_train/batch_0"] == golden["cnn2d_forward_train/T_short"] == _lib.E_BAD_SHAPE
