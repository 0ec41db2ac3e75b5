"""The DeepfakeDetector training step on the GPU (dfa_dlq_forward_train / dfa_dlq_backward, DlqTrainer, dfa_amd.train_dlqueen) against
the float64 oracle tests/dlqueen_train_oracle.py.

Bounds: the project's rule of tests/test_train_saturated_gpu.py -- per element max(2e-4, 8 * floor_max) of the tensor's scale and
max(1e-4, 8 * floor_L2) in relative L2, floor = the float32 CPU oracle's distance from float64, never the GPU's output.  GELU is
smooth: no ReLU-flip allowance.  The conv biases in front of a BatchNorm (true gradient zero): |db| <= 1e-4 max|dW| + 1e-6."""
import ctypes as C
import functools
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import dlqueen_train_oracle as O
from saturated_train_states import _assert_row, print_tight_log, tight_deviation

pytestmark = pytest.mark.gpu
NOISE = {"enc.net.0.bias", "enc.net.4.bias", "enc.net.8.bias"}
BNS = ("enc.net.1", "enc.net.5", "enc.net.9")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _model(C_in, dropout=0.0, sd=None):
    from dfa_amd.dlqueen_model import DeepfakeDetector
    sd = O.make_state_dict(DeepfakeDetector, C_in) if sd is None else sd
    m = DeepfakeDetector(C_in, dropout=dropout)
    m.load_state_dict({k: v.clone() for k, v in sd.items()})
    return m.to("cuda"), sd


@functools.lru_cache(maxsize=None)
def _sd(C_in):
    from dfa_amd.dlqueen_model import DeepfakeDetector
    return O.make_state_dict(DeepfakeDetector, C_in)


def _gpu(x):
    """the batch on the GPU in the stored layout (rows padded to 16 bytes), what lies behind an utterance's end kept as it is"""
    from dfa_amd import _lib
    return _lib.stored_layout(x.to("cuda"), False, time_last=True)


def _raw_step(name, p=0.0, seed=5, offset=0, momentum=0.1):
    """forward_train -> loss -> backward straight on the C ABI; everything it left, on the host"""
    from dfa_amd import _lib
    B, C_in, T, lengths = O.CASES[name]
    xc, lengths, y = O.make_case(name)
    x = _gpu(xc)
    m, _ = _model(C_in, p, _sd(C_in))
    ctx = _lib.Context.get(x.device)
    lib, h = ctx.lib, ctx.handle
    ctx.use_current_stream()
    ts = m._abi_tensors()
    ctx.owner_changed("dlq", m)
    _lib.check(h, lib.dfa_dlq_set_params(h, _lib.ptr_array(ts), len(ts), C_in, 256))
    ws = torch.empty(lib.dfa_dlq_train_workspace_bytes(h, B, T, C_in), dtype=torch.uint8, device="cuda")
    keep = torch.full((3 * B * 256 * T + B * 256,), 7, dtype=torch.uint8, device="cuda")
    logits = torch.empty(B, device="cuda")
    loss, dl = torch.empty(1, device="cuda"), torch.empty(B, device="cuda")
    grads = [torch.full_like(q, float("nan")) for q in m.parameters()]
    ln = np.asarray(lengths, dtype=np.int32)
    sb, sc, _ = x.stride()
    _lib.check(h, lib.dfa_dlq_forward_train(h, _lib.ptr(x), B, T, C_in, sb, sc, C.c_void_p(ln.ctypes.data), p, seed, offset, momentum, 1,
                                            _lib.ptr(logits), _lib.ptr(keep), _lib.ptr(ws), ws.numel()))
    _lib.check(h, lib.dfa_bce_pos_weight_fwd_bwd(h, _lib.ptr(logits), _lib.ptr(y.to("cuda")), O.POS_WEIGHT, B, _lib.ptr(loss), _lib.ptr(dl)))
    _lib.check(h, lib.dfa_dlq_backward(h, _lib.ptr(x), B, T, C_in, sb, sc, _lib.ptr(dl), _lib.ptr_array(grads), 16, _lib.ptr(ws), ws.numel()))
    torch.cuda.synchronize()
    sd = m.state_dict()
    return {"logits": logits.cpu().numpy(), "loss": float(loss.item()), "grads": [g.cpu().numpy() for g in grads],
            "keep": keep.cpu().numpy(), "rm": [sd[b + ".running_mean"].cpu().numpy() for b in BNS],
            "rv": [sd[b + ".running_var"].cpu().numpy() for b in BNS]}


def _want(name, p, masks):
    _, C_in, _, _ = O.CASES[name]
    x, lengths, y = O.make_case(name)
    return (O.step(_sd(C_in), x, lengths, y, p=p, masks=masks, dtype=torch.float64),
            O.step(_sd(C_in), x, lengths, y, p=p, masks=masks, dtype=torch.float32))


@functools.lru_cache(maxsize=None)
def _want_p0(name):
    return _want(name, 0.0, None)


def _check(tag, got, want, fp32, stats=None):
    rows = []
    named = [("logits", got["logits"], want["logits"], fp32["logits"]), ("loss", got["loss"], want["loss"], fp32["loss"])]
    for l in range(3):
        named.append((f"running_mean{l}", got["rm"][l], want["running_mean"][l], fp32["running_mean"][l]))
        named.append((f"running_var{l}", got["rv"][l], want["running_var"][l], fp32["running_var"][l]))
        if stats is not None:
            named.append((f"batch_mean{l}", stats[0][l], want["mean"][l], fp32["mean"][l]))
            named.append((f"batch_var{l}", stats[1][l], want["var"][l], fp32["var"][l]))
    for k, g, w, f in zip(O.PARAMS, got["grads"], want["grads"], fp32["grads"]):
        assert np.isfinite(g).all(), k
        if k not in NOISE:
            named.append((k, g, w, f))
    rows = [tight_deviation(g, w, f, n) for n, g, w, f in named]
    print_tight_log(tag, rows)
    for r in rows:
        print(f"[{tag}] {r[0]}: max/scale {r[1]:.2e} (floor {r[3]:.2e}) l2 {r[2]:.2e} (floor {r[4]:.2e})")
    for k, g in zip(O.PARAMS, got["grads"]):
        if k in NOISE:
            bound = 1e-4 * float(np.abs(want["grads"][O.PARAMS.index(k.replace("bias", "weight"))]).max()) + 1e-6
            print(f"[{tag}] {k}: max |db| {np.abs(g).max():.2e} (bound {bound:.2e})")
            assert np.abs(g).max() <= bound, (k, float(np.abs(g).max()), bound)
    for r in rows:
        _assert_row(r)


@pytest.mark.parametrize("name", ["A", "B", "C", "D"])
def test_step_matches_float64_oracle_without_dropout(name):
    B, _, T, lengths = O.CASES[name]
    got = _raw_step(name)
    one = _raw_step(name, momentum=1.0)          # momentum 1: the running statistics ARE the batch's (variance unbiased)
    N = B * T
    stats = (one["rm"], [v * (N - 1) / N for v in one["rv"]])
    want, fp32 = _want_p0(name)
    assert (got["keep"] == 1).all()
    _check(f"dlq train {name} p=0", got, want, fp32, stats)
    if 1 in lengths:     # the len = 1 utterance: its variance is exactly 0 < 1e-6, so its dstd path contributes exactly nothing
        b = lengths.index(1)
        assert (want["pool_var"][b] == 0).all()


@pytest.mark.parametrize("name", ["A", "C"])
def test_step_matches_float64_oracle_with_the_masks_it_applied(name):
    B, _, T, _ = O.CASES[name]
    p = 0.3
    got = _raw_step(name, p=p, seed=5, offset=0)
    keep = got["keep"]
    assert set(np.unique(keep)) <= {0, 1}
    n = keep.size
    assert abs(keep.mean() - 0.7) <= 5 * math.sqrt(0.21 / n), (keep.mean(), n)
    assert (_raw_step(name, p=p, seed=5, offset=977)["keep"] != keep).any()
    want, fp32 = _want(name, p, O.split_keep(keep, B, T))
    _check(f"dlq train {name} p=0.3", got, want, fp32)


def _trainer_steps(x, lengths, y, C_in, p, steps, before=None, ema=0.999, poison_ws=False):
    from dfa_amd.training import DlqTrainer
    m, _ = _model(C_in, p, _sd(C_in))
    m._drop_seed, m._drop_offset = 5, 0
    tr = DlqTrainer(m, lr=1e-3, weight_decay=1e-4, pos_weight=O.POS_WEIGHT, grad_clip=5.0, ema_decay=ema)
    out = []
    if poison_ws:        # the trainer reuses a workspace that is large enough: give it one, NaN-filled before every step
        from dfa_amd import _lib
        ctx = _lib.Context.get(x.device)
        m._train_ws = torch.empty(ctx.lib.dfa_dlq_train_workspace_bytes(ctx.handle, x.shape[0], x.shape[2], C_in), dtype=torch.uint8, device=x.device)
    for _ in range(steps):
        if before is not None:
            before()
        if poison_ws:
            m._train_ws.view(torch.float32)[:] = float("nan")
        loss = tr.step(x, lengths, y)
        out.append((loss.clone(), tr.flat_g.clone()))
    torch.cuda.synchronize()
    rv = torch.cat([m.state_dict()[b + ".running_var"] for b in BNS])
    return out, tr.flat_p.clone(), rv.clone(), tr.shadow.clone()


def _same(a, b, what):
    for (la, ga), (lb, gb) in zip(a[0], b[0]):
        assert torch.equal(la, lb), what + ": loss"
        assert torch.equal(ga, gb), what + ": flat_g"
    for u, v, n in zip(a[1:], b[1:], ("flat_p", "running_var", "ema shadow")):
        assert torch.equal(u, v), f"{what}: {n}"
        assert bool(torch.isfinite(u).all()), n


def test_step_ignores_padding_workspace_and_lds_contents():
    from dfa_amd import _lib
    _, C_in, _, _ = O.CASES["C"]
    x, lengths, y = O.make_case("C")
    xg = O.make_case("C", garbage=1e30)[0]
    clean = _trainer_steps(x.to("cuda"), lengths, y, C_in, 0.3, 3)
    _same(_trainer_steps(xg.to("cuda"), lengths, y, C_in, 0.3, 3), clean, "finite garbage behind the utterances")
    _same(_trainer_steps(x.to("cuda"), lengths, y, C_in, 0.3, 3, poison_ws=True), clean, "NaN-filled workspace")
    ctx = _lib.Context.get(torch.device("cuda"))
    for pat in (0xFFFFFFFF, 0x7FC00000):
        _same(_trainer_steps(x.to("cuda"), lengths, y, C_in, 0.3, 3, before=lambda: ctx.set_option("poison_lds", pat)), clean,
              f"poison_lds {pat:#x}")


def test_three_steps_reproduce_bit_for_bit_at_size():
    g = torch.Generator().manual_seed(3)
    B, C_in, T = 32, 180, 321
    x = (torch.randn((B, C_in, 324), generator=g) * 3.2 - 0.07)[:, :, :T]
    lengths = [321] + [int(v) for v in torch.randint(161, 322, (B - 1,), generator=g)]
    for b, n in enumerate(lengths):
        x[b, :, n:] = float("nan")
    y = torch.tensor([float(b % 2) for b in range(B)])
    xd = x.to("cuda")
    _same(_trainer_steps(xd, lengths, y, C_in, 0.3, 3), _trainer_steps(xd, lengths, y, C_in, 0.3, 3), "second run")


def test_trainer_step_clips_updates_and_keeps_an_ema():
    from dfa_amd.training import DlqTrainer
    B, C_in, T, _ = O.CASES["A"]
    x, lengths, y = O.make_case("A")
    want, _ = _want_p0("A")
    g64 = np.concatenate([g.reshape(-1) for g in want["grads"]])
    norm = float(np.sqrt((g64 ** 2).sum()))
    clip, lr, wd, decay = 0.5 * norm, 1e-3, 1e-4, 0.9
    m, sd = _model(C_in, 0.0, _sd(C_in))
    tr = DlqTrainer(m, lr=lr, weight_decay=wd, pos_weight=O.POS_WEIGHT, grad_clip=clip, ema_decay=decay)
    loss = tr.step(x.to("cuda"), lengths, y)
    assert abs(loss.item() - float(want["loss"])) <= 1e-5 * max(1.0, abs(float(want["loss"])))
    assert abs(tr.norm_buf.item() - norm) <= 2e-4 * norm
    gc = g64 * min(1.0, clip / (norm + 1e-6))
    p0 = np.concatenate([sd[k].double().numpy().reshape(-1) for k in O.PARAMS])
    mh, vh = gc, gc * gc                                   # bias-corrected first-step moments
    p1 = p0 * (1 - lr * wd) - lr * mh / (np.sqrt(vh) + 1e-8)
    from test_train_shapes_gpu import _check_state
    got = {k: v.detach().clone() for k, v in m.state_dict().items()}
    wantsd, off = {}, 0
    for k in O.PARAMS:
        n = sd[k].numel()
        wantsd[k] = p1[off:off + n].reshape(sd[k].shape)
        off += n
    for l, b in enumerate(BNS):
        wantsd[b + ".running_mean"], wantsd[b + ".running_var"] = want["running_mean"][l], want["running_var"][l]
        wantsd[b + ".num_batches_tracked"] = 1
    _check_state(got, wantsd, sd, NOISE)
    ema = decay * p0 + (1 - decay) * tr.flat_p.double().cpu().numpy()
    np.testing.assert_allclose(tr.shadow.cpu().numpy(), ema, rtol=1e-6, atol=1e-7)
    # eval after the step runs on the NEW weights (the prepared images were invalidated)
    import dlqueen_oracle as EO
    xe = torch.where(torch.isnan(x), torch.zeros(()), x)
    lg = m.eval()(xe.to("cuda"), lengths).cpu().numpy()
    new = EO.forward({k: v.cpu() for k, v in m.state_dict().items()}, xe, lengths)[0]
    old = EO.forward(sd, xe, lengths)[0]
    np.testing.assert_allclose(lg, new, atol=2e-4, rtol=1e-4)
    assert np.abs(new - old).max() > 10 * np.abs(lg - new).max()
    with tr.ema_applied():
        le = m(xe.to("cuda"), lengths).cpu().numpy()
    assert np.abs(le - lg).max() > 0 and torch.equal(m(xe.to("cuda"), lengths).cpu(), torch.from_numpy(lg))


def test_abi_refusals_name_the_argument_and_leave_the_gradients():
    from dfa_amd import _lib
    B, C_in, T, lengths = O.CASES["B"]
    x, lengths, y = O.make_case("B")
    x = _gpu(x)
    m, _ = _model(C_in)
    ctx = _lib.Context.get(x.device)
    lib, h = ctx.lib, ctx.handle
    ctx.use_current_stream()
    ts = m._abi_tensors()
    ctx.owner_changed("dlq", m)
    _lib.check(h, lib.dfa_dlq_set_params(h, _lib.ptr_array(ts), len(ts), C_in, 256))
    nbytes = lib.dfa_dlq_train_workspace_bytes(h, B, T, C_in)
    assert lib.dfa_dlq_train_workspace_bytes(h, 1, 1, C_in) == 0
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    logits, dl = torch.empty(B, device="cuda"), torch.zeros(B, device="cuda")
    grads = [torch.full_like(q, 3.0) for q in m.parameters()]
    sb, sc, _ = x.stride()

    def fwd(B_=B, T_=T, C_=C_in, ln=lengths, sb_=sb, sc_=sc, nb=nbytes):
        ln = np.asarray(ln, dtype=np.int32)
        return lib.dfa_dlq_forward_train(h, _lib.ptr(x), B_, T_, C_, sb_, sc_, C.c_void_p(ln.ctypes.data), 0.0, 1, 0, 0.1, 1, _lib.ptr(logits),
                                         None, _lib.ptr(ws), nb)

    def bwd(B_=B, n=16, C_=C_in):
        return lib.dfa_dlq_backward(h, _lib.ptr(x), B_, T, C_, sb, sc, _lib.ptr(dl), _lib.ptr_array(grads), n, _lib.ptr(ws), nbytes)

    def refused(code, want, *words):
        msg = lib.dfa_last_error(h).decode()
        assert code == want, (code, msg)
        for w in words:
            assert w in msg, (w, msg)

    refused(fwd(C_=C_in + 4), _lib.E_BAD_SHAPE, "in_ch")
    refused(fwd(B_=0), _lib.E_BAD_SHAPE, "B=0")
    refused(fwd(B_=1, T_=1, ln=[1]), _lib.E_BAD_SHAPE, "B * T_max")
    refused(fwd(ln=[5, 6]), _lib.E_BAD_SHAPE, "lengths[1]=6")
    refused(fwd(ln=[0, 2]), _lib.E_BAD_SHAPE, "lengths[0]=0")
    refused(fwd(sc_=sc + 1), _lib.E_UNSUPPORTED, "stride_c")
    refused(fwd(nb=nbytes - 256), _lib.E_WORKSPACE, "workspace too small")
    refused(bwd(), _lib.E_NOT_PREPARED, "dfa_dlq_forward_train")           # every forward above was refused: none is in flight
    buf = torch.zeros(1024, device="cuda")
    fn = _lib.BnSync.FN(lambda *_: 0)
    _lib.check(h, lib.dfa_ctx_set_bn_sync(h, C.cast(fn, C.c_void_p), None, 2, C.c_void_p(buf.data_ptr()), buf.numel()))
    try:
        refused(fwd(), _lib.E_UNSUPPORTED, "dfa_ctx_set_bn_sync")
    finally:
        _lib.check(h, lib.dfa_ctx_set_bn_sync(h, None, None, 1, None, 0))
    graph = torch.cuda.CUDAGraph()
    with pytest.raises(ValueError, match="captured"):           # refused before anything is launched or allocated
        with torch.cuda.graph(graph):
            ctx.use_current_stream()
            _lib.check(h, fwd())
    torch.cuda.synchronize()
    ctx.use_current_stream()
    assert fwd() == 0, lib.dfa_last_error(h).decode()
    refused(bwd(n=15), _lib.E_BAD_SHAPE, "16", "15")
    refused(bwd(B_=B + 1), _lib.E_NOT_PREPARED, "dfa_dlq_forward_train")
    refused(bwd(C_=C_in - 4), _lib.E_NOT_PREPARED, "dfa_dlq_forward_train")  # another in_ch than the forward's (a smaller plan)
    torch.cuda.synchronize()
    assert all(bool((g == 3.0).all()) for g in grads)                      # no refused call wrote a gradient
    assert bwd() == 0, lib.dfa_last_error(h).decode()                      # and the next valid one succeeds
    torch.cuda.synchronize()
    assert all(bool(torch.isfinite(g).all()) and not bool((g == 3.0).all()) for g in grads)
    _lib.check(h, lib.dfa_dlq_set_params(h, _lib.ptr_array(ts), len(ts), C_in, 256))
    refused(bwd(), _lib.E_NOT_PREPARED, "dfa_dlq_forward_train")           # set_params ends the batch in flight
    assert fwd() == 0 and bwd() == 0, lib.dfa_last_error(h).decode()       # and the next pair runs
    torch.cuda.synchronize()
    hh = C.c_void_p()
    assert lib.dfa_ctx_create(ctx.index, None, C.byref(hh)) == 0             # parameters not set: a context of its own
    try:
        ln = np.asarray(lengths, dtype=np.int32)
        code = lib.dfa_dlq_forward_train(hh, _lib.ptr(x), B, T, C_in, sb, sc, C.c_void_p(ln.ctypes.data), 0.0, 1, 0, 0.1, 1, _lib.ptr(logits), None,
                                         _lib.ptr(ws), nbytes)
        assert code == _lib.E_NOT_PREPARED and "dfa_dlq_set_params" in lib.dfa_last_error(hh).decode()
    finally:
        lib.dfa_ctx_destroy(hh)


def _make_data(root, n=48, C_in=180):
    import pandas as pd
    g = np.random.default_rng(0)
    for split in ("train", "dev"):
        os.makedirs(os.path.join(root, split))
        ids = [f"{split}{i:03d}" for i in range(n)]
        labels = [int(i % 3 == 0) for i in range(n)]
        feats = [(g.standard_normal((C_in, int(g.integers(40, 131)))) * 3 + (0.8 if lab else -0.8)).astype(np.float32) for lab in labels]
        pd.DataFrame({"uttid": ids, "features": feats}).to_pickle(os.path.join(root, split, "features.pkl"))
        pd.DataFrame({"uttid": ids, "label": labels}).to_pickle(os.path.join(root, split, "labels.pkl"))


def test_train_cli_end_to_end(tmp_path):
    from dfa_amd.dlqueen_model import DeepfakeDetector
    data = str(tmp_path / "data")
    _make_data(data)
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    blobs = []
    for run in range(2):
        os.makedirs(tmp_path / f"run{run}")
        ckpt = str(tmp_path / f"run{run}" / "best.pth")          # the same file name: torch.save writes it into the archive
        r = subprocess.run([sys.executable, "-m", "dfa_amd.train_dlqueen", "--data_dir", data, "--train_split", "train", "--dev_split", "dev",
                            "--ckpt_path", ckpt, "--epochs", "2", "--batch_size", "8", "--dropout", "0.3", "--ema", "--specaug", "--seed", "7"],
                           capture_output=True, text=True, env=env, cwd=ROOT, timeout=600)
        assert r.returncode == 0, r.stdout + r.stderr
        losses = [float(line.split("train_loss=")[1].split()[0]) for line in r.stdout.splitlines() if "train_loss=" in line]
        assert len(losses) == 2 and all(math.isfinite(v) for v in losses), r.stdout
        blobs.append(open(ckpt, "rb").read())
    assert blobs[0] == blobs[1], "same seed, different checkpoint"
    sd = torch.load(ckpt, map_location="cpu")
    ref = DeepfakeDetector(180).state_dict()
    assert list(sd.keys()) == list(ref.keys())
    assert all(sd[k].shape == ref[k].shape and sd[k].dtype == ref[k].dtype for k in ref)
    pred = str(tmp_path / "pred.pkl")
    r = subprocess.run([sys.executable, "-m", "dfa_amd.dlqueen_model", "--data_dir", data, "--test_split", "dev", "--ckpt_path", ckpt,
                        "--prediction_pkl", pred], capture_output=True, text=True, env=env, cwd=ROOT, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    import pandas as pd
    out = pd.read_pickle(pred)
    assert len(out) == 48 and np.isfinite(out["predictions"].to_numpy()).all()
