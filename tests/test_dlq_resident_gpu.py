"""The DeepfakeDetector's resident training set on the GPU: dfa_dlq_gather_batch, DlqResidentSet,
resident_epoch_batches, run_inference_resident and `train_dlqueen --resident` against the existing host loop, which is the
oracle.  The host keeps the sampler and the random draws, so every comparison is exact: torch.equal / np.array_equal."""
import ctypes as C
import functools
import os
import random
import subprocess
import sys

import numpy as np
import pytest
import torch

import dlqueen_train_oracle as O

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# lengths around the 4-frame slot (1..9), the 64-frame tile (63..65) and the 64-lane wave in slots (255..257 frames); 321 = the reference's
LENGTHS = [1, 2, 3, 4, 5, 7, 8, 9, 63, 64, 65, 130, 255, 256, 257, 321]
NAN, INF = float("nan"), float("inf")


@functools.lru_cache(maxsize=None)
def _stub(Cc):
    """(features, labels, sampling order with repeats, the resident set): 16 utterances, one per length, in a shuffled order"""
    from dfa_amd.dataloaders import DlqResidentSet
    g = torch.Generator().manual_seed(100 + Cc)
    r = random.Random(Cc)
    lens = LENGTHS[:]
    r.shuffle(lens)
    feats = [torch.randn(Cc, T, generator=g) + 0.25 for T in lens]
    labels = np.array([i % 3 == 0 for i in range(len(lens))], dtype=int)
    order = list(range(len(lens)))
    r.shuffle(order)
    order += [r.randrange(len(lens)) for _ in range(21)]          # 37 draws: sampling is with replacement
    return feats, labels, order, DlqResidentSet(feats, labels, device="cuda", chunk_utts=5)


def _expected(feats, idx, spans=None, n_t=0):
    """the defining expression on the host: [b, C, T_pad] zero outside the utterances and inside the spans"""
    lens = [int(feats[i].shape[-1]) for i in idx]
    T_pad = -(-max(lens) // 4) * 4
    out = torch.zeros(len(idx), feats[0].shape[0], T_pad)
    for j, i in enumerate(idx):
        u = feats[i].clone()
        if spans is not None:
            for k, (s0, w) in enumerate(np.asarray(spans[j]).tolist()):
                if k < n_t:
                    u[:, s0:s0 + w] = 0.0
                else:
                    u[s0:s0 + w, :] = 0.0
        out[j, :, :lens[j]] = u
    return out


@pytest.mark.parametrize("specaug", [None, (2, 2, 3, 1), (400, 3, 400, 3)], ids=["plain", "small", "whole_axis"])
@pytest.mark.parametrize("bs", [1, 5, 16])
@pytest.mark.parametrize("Cc", [180, 5])
def test_gather_parity_with_host_loop(Cc, bs, specaug):
    from dfa_amd import train_dlqueen as TD
    from dfa_amd.dlqueen_model import DeepfakeDetector
    feats, labels, order, rset = _stub(Cc)
    assert rset.bytes_resident == 4 * rset.total_floats and np.array_equal(rset.lengths, [f.shape[-1] for f in feats])
    ra, rb = random.Random(9), random.Random(9)
    host = TD.epoch_batches(feats, labels, order, bs, specaug, ra)
    res = TD.resident_epoch_batches(rset, order, bs, specaug, rb)
    n = 0
    for (xh, lh, yh), (xr, lr, yr) in zip(host, res):
        assert xr.is_cuda and yr.is_cuda and xr.dtype == torch.float32 and yr.dtype == torch.float32
        assert tuple(xr.shape) == tuple(xh.shape) and DeepfakeDetector._conforms(xr)
        assert lr.dtype == np.int32 and np.array_equal(lr, lh)
        assert torch.equal(xr, xh.to("cuda")), (n, int((xr.cpu() != xh).sum()))
        assert torch.equal(yr, yh.to("cuda"))
        n += 1
    assert n == -(-len(order) // bs)
    assert next(host, None) is None and next(res, None) is None
    assert ra.random() == rb.random()


def test_padding_and_stale_bytes_are_inputs():
    from dfa_amd import _lib
    from dfa_amd.dataloaders import DlqResidentSet
    feats, _, _, _ = _stub(5)
    rset = DlqResidentSet(feats, None, device="cuda")                   # a set of its own: this test writes into it
    lens = [int(f.shape[-1]) for f in feats]
    idx = [lens.index(130), lens.index(7), lens.index(321), lens.index(130), lens.index(1)]
    n_t = 1
    spans = np.array([[[10, 20], [2, 2]], [[0, 7], [0, 0]], [[300, 21], [4, 1]], [[0, 0], [0, 5]], [[0, 1], [1, 3]]], dtype=np.int32)
    want = _expected(feats, idx, spans, n_t)
    for i in range(len(feats)):                                         # NaN in every row's padding floats
        pitch = -(-lens[i] // 4) * 4
        rows = rset.set[int(rset.offsets[i]):int(rset.offsets[i]) + 5 * pitch].view(5, pitch)
        rows[:, lens[i]:] = NAN
    i130 = lens.index(130)                                              # NaN / Inf where the spans of batch item 0 mask
    rows = rset.set[int(rset.offsets[i130]):int(rset.offsets[i130]) + 5 * 132].view(5, 132)
    rows[:, 10:30] = NAN
    rows[2:4, :] = INF
    rset.batch(idx, spans, n_t)
    rset._x.fill_(NAN)                                                  # the batch buffer needs no memset
    x, lengths, y = rset.batch(idx, spans, n_t)
    assert y is None and np.array_equal(lengths, [130, 7, 321, 130, 1])
    full = torch.as_strided(x, (5, 5, 324), x.stride())                 # all T_pad columns of every row
    assert bool(torch.isfinite(full).all()) and torch.equal(full.cpu(), want)
    assert not bool(torch.signbit(full).logical_and(full == 0).any())   # an exact +0.0

    # a batch buffer larger than needed: stride_c = T_pad + 8, stride_b with slack, guard floats before and after
    ctx = rset.ctx
    B, Cc, T, T_pad = 5, 5, 321, 324
    sc, guard = T_pad + 8, 64
    sb = Cc * sc + 12
    big = torch.full((guard + B * sb + guard,), NAN, device="cuda")
    tab = torch.empty(ctx.lib.dfa_dlq_gather_workspace_bytes(B, 1, 1), dtype=torch.uint8, device="cuda")
    src = np.ascontiguousarray(rset.offsets[idx])
    ln = np.ascontiguousarray(rset.lengths[idx])
    ctx.use_current_stream()
    code = ctx.lib.dfa_dlq_gather_batch(ctx.handle, _lib.ptr(rset.set), rset.total_floats, C.c_void_p(src.ctypes.data), C.c_void_p(ln.ctypes.data),
                                        C.c_void_p(spans.ctypes.data), 1, 1, B, T, Cc, C.c_void_p(big.data_ptr() + 4 * guard), sb, sc,
                                        _lib.ptr(tab), tab.numel())
    assert code == 0, ctx.lib.dfa_last_error(ctx.handle).decode()
    host = big.cpu()
    written = torch.zeros_like(host, dtype=torch.bool)
    region = torch.as_strided(written, (B, Cc, T_pad), (sb, sc, 1), guard)
    region[:] = True
    assert torch.equal(torch.as_strided(host, (B, Cc, T_pad), (sb, sc, 1), guard), want)
    assert bool(torch.isnan(host[~written]).all()) and int((~written).sum()) == 2 * guard + B * sb - B * Cc * T_pad


def test_abi_refusals_leave_the_context_usable():
    from dfa_amd import _lib
    feats, _, _, rset = _stub(5)
    ctx = rset.ctx
    lib, h = ctx.lib, ctx.handle
    lens = [int(f.shape[-1]) for f in feats]
    idx = [lens.index(9), lens.index(65), lens.index(3)]
    B, Cc, T, T_pad = 3, 5, 65, 68
    spans0 = np.array([[[1, 2], [0, 1]], [[60, 5], [3, 2]], [[0, 0], [0, 0]]], dtype=np.int32)
    want = _expected(feats, idx, spans0, 1)
    xbuf = torch.full((B * Cc * T_pad + 4,), NAN, device="cuda")
    tab = torch.empty(4096 + 256, dtype=torch.uint8, device="cuda")
    need = lib.dfa_dlq_gather_workspace_bytes(B, 1, 1)
    ctx.use_current_stream()

    def call(**kw):
        a = dict(h=h, set=rset.set.data_ptr(), set_floats=rset.total_floats, src=np.ascontiguousarray(rset.offsets[idx]),
                 ln=np.ascontiguousarray(rset.lengths[idx]), spans=spans0, n_t=1, n_f=1, B=B, T=T, C=Cc, x=xbuf.data_ptr(), sb=Cc * T_pad,
                 sc=T_pad, ws=tab.data_ptr(), ws_bytes=need)
        a.update(kw)
        keep = [np.ascontiguousarray(a[k]) if a[k] is not None else None for k in ("src", "ln", "spans")]
        p = [C.c_void_p(v.ctypes.data) if v is not None else None for v in keep]
        return lib.dfa_dlq_gather_batch(a["h"], C.c_void_p(a["set"]) if a["set"] else None, a["set_floats"], p[0], p[1], p[2], a["n_t"], a["n_f"],
                                        a["B"], a["T"], a["C"], C.c_void_p(a["x"]) if a["x"] else None, a["sb"], a["sc"],
                                        C.c_void_p(a["ws"]) if a["ws"] else None, a["ws_bytes"])

    def refused(code, want_code, *words):
        msg = lib.dfa_last_error(h).decode()
        assert code == want_code, (code, msg)
        for w in words:
            assert w in msg, (w, msg)

    def edit(arr, pos, val):
        out = np.array(arr)
        out[pos] = val
        return out

    src, ln = rset.offsets[idx], rset.lengths[idx]
    assert call(h=None) == _lib.E_NULL_PTR                                                   # no context: a code, no text
    for name in ("set", "src", "ln", "x", "ws"):
        refused(call(**{name: None}), _lib.E_NULL_PTR, "non-null")
    refused(call(spans=None), _lib.E_NULL_PTR, "spans")
    refused(call(B=0), _lib.E_BAD_SHAPE, "batch", "0")
    refused(call(C=0), _lib.E_BAD_SHAPE, "C must be")
    refused(call(ln=edit(ln, 1, 0)), _lib.E_BAD_SHAPE, "lengths[1]=0")
    refused(call(ln=edit(ln, 2, T + 1)), _lib.E_BAD_SHAPE, "lengths[2]=66")
    refused(call(src=edit(src, 1, -4)), _lib.E_BAD_SHAPE, "src_off[1]=-4")
    refused(call(src=edit(src, 2, int(src[2]) + 2)), _lib.E_BAD_SHAPE, f"src_off[2]={int(src[2]) + 2}")
    refused(call(src=edit(src, 0, rset.total_floats - 4 * Cc * 3 + 4)), _lib.E_BAD_SHAPE, "src_off[0]=", "set_floats")
    refused(call(set_floats=int(src.max())), _lib.E_BAD_SHAPE, "src_off[", "set_floats")
    refused(call(spans=edit(spans0, (1, 0, 0), -1)), _lib.E_BAD_SHAPE, "time span 0 of utterance 1")
    refused(call(spans=edit(spans0, (0, 0, 1), -2)), _lib.E_BAD_SHAPE, "time span 0 of utterance 0")
    refused(call(spans=edit(spans0, (2, 0), (2, 2))), _lib.E_BAD_SHAPE, "time span 0 of utterance 2")   # start + width = 4 > its 3 frames
    refused(call(spans=edit(spans0, (1, 1), (4, 2))), _lib.E_BAD_SHAPE, "channel span 0 of utterance 1")
    refused(call(spans=edit(spans0, (0, 1, 0), -1)), _lib.E_BAD_SHAPE, "channel span 0 of utterance 0")
    refused(call(x=xbuf.data_ptr() + 4), _lib.E_BAD_SHAPE, "x must be 16-byte aligned")
    refused(call(sb=Cc * T_pad + 2), _lib.E_BAD_SHAPE, "stride_b")
    refused(call(sc=T_pad + 2, sb=Cc * (T_pad + 4)), _lib.E_BAD_SHAPE, "stride_c")
    refused(call(sc=T_pad - 4), _lib.E_BAD_SHAPE, "stride_c", "T_pad=68")
    refused(call(ws_bytes=need - 1), _lib.E_WORKSPACE, "too small")
    refused(call(ws=tab.data_ptr() + 16), _lib.E_WORKSPACE, "256-byte aligned")
    many = np.zeros((B, 17, 2), dtype=np.int32)
    refused(call(spans=many, n_t=9, n_f=8, ws_bytes=4096), _lib.E_UNSUPPORTED, "17")
    torch.cuda.synchronize()
    assert bool(torch.isnan(xbuf).all())                                                     # no refused call launched anything
    assert call() == 0, lib.dfa_last_error(h).decode()                                       # and the next valid one succeeds
    assert torch.equal(xbuf[:B * Cc * T_pad].view(B, Cc, T_pad).cpu(), want) and bool(torch.isnan(xbuf[B * Cc * T_pad:]).all())

    # a capturing stream: the table is per-call data.  Refused before anything is launched or recorded.
    rset.batch(idx, spans0, 1)
    rset._x.fill_(NAN)
    g = torch.cuda.CUDAGraph()
    with pytest.raises(ValueError, match="captured"):
        with torch.cuda.graph(g):
            rset.batch(idx, spans0, 1)
    torch.cuda.synchronize()
    assert bool(torch.isnan(rset._x).all())
    x, _, _ = rset.batch(idx, spans0, 1)                                                      # the stream is usable afterwards
    assert torch.equal(x.cpu(), want[:, :, :T])


def test_step_reads_the_resident_batch_in_place():
    from dfa_amd import train_dlqueen as TD
    from dfa_amd.dataloaders import DlqResidentSet
    from dfa_amd.dlqueen_model import DeepfakeDetector
    from dfa_amd.training import DlqTrainer
    g = torch.Generator().manual_seed(3)
    feats = [torch.randn(180, T, generator=g) * 2 + 0.1 for T in (37, 1, 20, 36)]
    labels = np.array([1, 0, 0, 1])
    rset = DlqResidentSet(feats, labels, device="cuda")
    sd = O.make_state_dict(DeepfakeDetector, 180)
    specaug, order = (2, 2, 3, 1), [0, 1, 2, 3]
    left = {}
    for path in ("host", "resident"):
        m = DeepfakeDetector(180, dropout=0.3)
        m.load_state_dict({k: v.clone() for k, v in sd.items()})
        m = m.to("cuda")
        m._drop_seed, m._drop_offset = 11, 0
        tr = DlqTrainer(m, lr=1e-3, pos_weight=2.0, grad_clip=0.0)
        rng = random.Random(4)
        if path == "host":
            xh, lengths, y = next(TD.epoch_batches(feats, labels, order, 4, specaug, rng))
            x = xh.to("cuda")
        else:
            x, lengths, y = next(TD.resident_epoch_batches(rset, order, 4, specaug, rng))
            assert DeepfakeDetector._conforms(x) and x.data_ptr() == rset._x.data_ptr()
        assert tuple(x.shape) == (4, 180, 37) and lengths.tolist() == [37, 1, 20, 36]
        loss = tr.step(x, lengths, y)
        left[path] = [loss.clone(), tr.logits.clone()] + [v.clone() for v in tr.grad_views]
        assert len(tr.grad_views) == 16 and all(bool(torch.isfinite(v).all()) for v in left[path])
    for k, (a, b) in enumerate(zip(left["host"], left["resident"])):
        assert torch.equal(a, b), (k, float((a - b).abs().max()))


def test_resident_inference_equals_file_order_inference():
    from dfa_amd.dataloaders import DlqResidentSet
    from dfa_amd.dlqueen_model import DeepfakeDetector, evaluate_eer, evaluate_eer_resident, run_inference, run_inference_resident
    g = torch.Generator().manual_seed(8)
    feats = [torch.randn(180, T, generator=g) * 2 + (0.5 if i % 2 else -0.5) for i, T in enumerate((40, 77, 5, 130, 64, 65, 1, 99, 128, 12, 33))]
    labels = np.array([i % 2 for i in range(11)])
    m = DeepfakeDetector(180)
    m.load_state_dict(O.make_state_dict(DeepfakeDetector, 180))
    m = m.to("cuda").eval()
    rset = DlqResidentSet(feats, None, device="cuda", chunk_utts=4)
    want = run_inference(m, feats, 4, device="cuda", file_order=True)
    got = run_inference_resident(m, rset, 4)
    assert got.shape == (11,) and torch.equal(got, want) and bool(torch.isfinite(got).all())
    assert torch.equal(run_inference_resident(m, rset, 4, use_prob=True), torch.sigmoid(want))
    assert evaluate_eer_resident(m, rset, labels, 4) == evaluate_eer(m, feats, labels, 4, device="cuda", file_order=True)


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


def test_train_cli_resident_equals_host_loop(tmp_path):
    data = str(tmp_path / "data")
    _make_data(data)
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    lines, states = [], []
    for flags in ([], ["--resident"]):
        ckpt = str(tmp_path / f"best{len(flags)}.pth")
        r = subprocess.run([sys.executable, "-m", "dfa_amd.train_dlqueen", "--data_dir", data, "--train_split", "train", "--dev_split", "dev",
                            "--ckpt_path", ckpt, "--epochs", "2", "--batch_size", "8", "--dropout", "0.3", "--ema", "--specaug", "--seed", "7"]
                           + flags, capture_output=True, text=True, env=env, cwd=ROOT, timeout=600)
        assert r.returncode == 0, r.stdout + r.stderr
        lines.append([ln for ln in r.stdout.splitlines() if ln.startswith("Epoch ")])
        states.append(torch.load(ckpt, map_location="cpu"))
    assert len(lines[0]) == 2 and lines[0] == lines[1], lines              # loss and dev EER, as printed
    assert list(states[0].keys()) == list(states[1].keys())
    for k in states[0]:
        assert torch.equal(states[0][k], states[1][k]), k
