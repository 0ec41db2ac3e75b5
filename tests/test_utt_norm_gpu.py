"""Per-utterance CMN / CVMN normalisation on the GPU: dfa_utt_norm in both layout forms and
dfa_utt_norm_packed against the float64 oracle (tests/utt_norm_oracle.py) at its per-row bound, the bit-for-bit promise (a row's
output is a function of its n values, n and the mode), every refusal, and the wiring: ResidentBatcher(norm=), DlqResidentSet(norm=)
and predict_scores_ragged(norm=).  Inputs, lengths (around the 16-byte piece, the 64-lane wave, the wave in pieces, the reference's
321 and one frame past the on-chip row cap) and the bound come from the oracle module; each expectation is computed once."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import utt_norm_oracle as UO

pytestmark = pytest.mark.gpu
NAN = float("nan")
FORMS = ("time", "feat")
CODES = {"cmn": 1, "cvmn": 2}


def _bits(t):
    return t.detach().cpu().contiguous().numpy().view(np.int32)


def _ctx():
    from dfa_amd import _lib
    return _lib.Context.get(torch.device("cuda", 0))


def _batch(utts, form, T_max=None, extra_pitch=0, behind=NAN, order=None):
    """The utterances ([C, T_i] numpy) as one padded batch x [B, T_max, C] on the GPU in the layout `form`, `behind` in every
    float that is not an utterance's (padding frames and, in the time form, the pitch): (x, lengths)"""
    order = list(range(len(utts))) if order is None else order
    utts = [utts[i] for i in order]
    lens = [u.shape[1] for u in utts]
    T_max = max(lens) if T_max is None else T_max
    Cc = utts[0].shape[0]
    if form == "time":
        pitch = -(-T_max // 4) * 4 + extra_pitch
        host = torch.full((len(utts), Cc, pitch), behind)
        for j, u in enumerate(utts):
            host[j, :, :lens[j]] = torch.from_numpy(np.array(u))
        return host.to("cuda").transpose(1, 2)[:, :T_max], lens
    host = torch.full((len(utts), T_max, Cc + extra_pitch), behind)
    for j, u in enumerate(utts):
        host[j, :lens[j], :Cc] = torch.from_numpy(np.array(u)).t()
    return host.to("cuda")[:, :, :Cc], lens


def _alone(u, form, mode):
    """utterance u [C, T] normalised by itself (B = 1, T_max = T, tight pitch, lengths = None) -> [C, T] on the host"""
    from dfa_amd.normalization import normalize_batch
    x, _ = _batch([u], form)
    return normalize_batch(x, mode)[0].t().cpu()


@functools.lru_cache(maxsize=None)
def _alone_cached(Cc, T, form, mode):
    return _alone(UO.utterance(Cc, T), form, mode)


# 1 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Cc", UO.CHANNELS)
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("mode", UO.MODES)
def test_parity_with_the_oracle_at_every_length(mode, form, Cc):
    from dfa_amd.normalization import normalize_batch
    utts = [UO.utterance(Cc, T) for T in UO.LENGTHS]
    x, lens = _batch(utts, form)
    y = normalize_batch(x, mode, lens)
    assert y.shape == x.shape and y.stride() == x.stride() and y.data_ptr() != x.data_ptr()
    got = y.cpu()
    for j, T in enumerate(UO.LENGTHS):
        y64, bound = UO.expected(Cc, T, mode)
        err = np.abs(got[j, :T].t().numpy().astype(np.float64) - y64).max(axis=1)
        print(f"{mode} {form} C={Cc} T={T}: max err / bound = {(err / bound).max():.4f}")
        assert (err <= bound).all(), (T, float((err / bound).max()))
        assert not _bits(got[j, T:]).any(), T                          # +0.0 behind the utterance, by bit pattern


# 2 ------------------------------------------------------------------------------------------------------------------------------
GROUPS = ((2, 3, 4, 5, 63), (64, 65, 255, 256, 257), (321, UO.HELD_FRAMES + 1, 5, 64, 257))


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("mode", UO.MODES)
def test_a_row_is_a_function_of_its_own_values(mode, form):
    from dfa_amd import _lib
    from dfa_amd.normalization import normalize_batch
    ctx = _ctx()
    for Cc in UO.CHANNELS:
        for g, group in enumerate(GROUPS):
            utts = [UO.utterance(Cc, T) for T in group]
            order = [3, 0, 4, 2, 1]
            # another position, a larger T_max, a larger pitch, NaN (g even) or finite garbage (g odd) behind every utterance
            x, lens = _batch(utts, form, T_max=max(group) + 7, extra_pitch=8, behind=NAN if g % 2 == 0 else 1e30, order=order)
            keep = x.clone()
            y = normalize_batch(x, mode, lens)
            assert torch.equal(_as_bits(x), _as_bits(keep))            # out of place: x is not written
            got = y.cpu()
            for j, i in enumerate(order):
                T = group[i]
                assert np.array_equal(_bits(got[j, :T].t()), _bits(_alone_cached(Cc, T, form, mode))), (Cc, T)
                assert not _bits(got[j, T:]).any(), (Cc, T)
            # in place, and through the ABI with a workspace full of NaN
            z = normalize_batch(x, mode, lens, out=x)
            assert z is x and np.array_equal(_bits(x), _bits(got))
            x2, _ = _batch(utts, form, T_max=max(group) + 7, extra_pitch=8, behind=NAN if g % 2 == 0 else 1e30, order=order)
            ws = torch.full((ctx.lib.dfa_utt_norm_workspace_bytes(len(lens)) // 4,), NAN, device="cuda")
            ln = np.asarray(lens, dtype=np.int32)
            ctx.use_current_stream()
            code = ctx.lib.dfa_utt_norm(ctx.handle, CODES[mode], _lib.ptr(x2), _lib.ptr(x2), *x2.shape[:2], Cc, *x2.stride(),
                                        C.c_void_p(ln.ctypes.data), _lib.ptr(ws), ws.numel() * 4)
            assert code == 0, ctx.lib.dfa_last_error(ctx.handle).decode()
            assert np.array_equal(_bits(x2), _bits(got))
        # lengths = None against lengths = [T] * B
        for T in (5, 257):
            x, lens = _batch([UO.utterance(Cc, T, seed=s) for s in range(3)], form)
            a, b = normalize_batch(x, mode), normalize_batch(x, mode, lens)
            assert np.array_equal(_bits(a), _bits(b)), (Cc, T)
            assert np.array_equal(_bits(a[0].t()), _bits(_alone_cached(Cc, T, form, mode)))


def _as_bits(t):
    return t.contiguous().view(torch.int32)


# 3 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Cc", UO.CHANNELS)
@pytest.mark.parametrize("mode", UO.MODES)
def test_packed_form_equals_the_batch_form(mode, Cc):
    from dfa_amd.dataloaders import plan_packed_set
    from dfa_amd.normalization import normalize_packed_
    lens = list(UO.LENGTHS[::-1])
    off, total = plan_packed_set(lens, Cc)
    host = torch.full((total,), NAN)
    for o, T in zip(off, lens):
        host[int(o):int(o) + Cc * (-(-T // 4) * 4)].view(Cc, -1)[:, :T] = torch.from_numpy(np.array(UO.utterance(Cc, T)))
    packed = host.to("cuda")
    assert normalize_packed_(packed, off, lens, Cc, mode) is packed
    got = packed.cpu()
    for o, T in zip(off, lens):
        rows = got[int(o):int(o) + Cc * (-(-T // 4) * 4)].view(Cc, -1)
        assert np.array_equal(_bits(rows[:, :T]), _bits(_alone_cached(Cc, T, "time", mode))), T
        assert not _bits(rows[:, T:]).any(), T                         # the pitch behind T_i: +0.0


# 4 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("mode", UO.MODES)
def test_constant_rows_give_exact_zeros(mode, form):
    from dfa_amd.normalization import normalize_batch
    lens = (2, 5, 321, UO.HELD_FRAMES + 1)
    utts = [np.stack([np.zeros(T, np.float32), np.full(T, 2.0, np.float32), np.zeros(T, np.float32), np.full(T, 2.0, np.float32)]) for T in lens]
    x, _ = _batch(utts, form)
    y = normalize_batch(x, mode, list(lens))
    assert not _bits(y).any()                                          # (2 - 2) / max(0, 1e-8) = +0.0


# 5 ------------------------------------------------------------------------------------------------------------------------------
def test_refusals_name_their_reason_and_write_nothing():
    from dfa_amd import _lib
    ctx = _ctx()
    lib, h = ctx.lib, ctx.handle
    B, T, Cc, P = 3, 10, 4, 12
    xs = torch.randn(B * Cc * P + 8, device="cuda")
    ys = torch.full((B * Cc * P + 8,), 7.0, device="cuda")
    ws = torch.empty(1024, dtype=torch.uint8, device="cuda")
    need = lib.dfa_utt_norm_workspace_bytes(B)
    assert 0 < need <= 512
    ctx.use_current_stream()

    def call(**kw):
        a = dict(h=h, mode=2, x=xs.data_ptr(), y=ys.data_ptr(), B=B, T=T, C=Cc, sb=Cc * P, st=1, sc=P, ln=[10, 7, 2], ws=ws.data_ptr(), nb=need)
        a.update(kw)
        ln = None if a["ln"] is None else np.asarray(a["ln"], dtype=np.int32)
        return lib.dfa_utt_norm(a["h"], a["mode"], C.c_void_p(a["x"]) if a["x"] else None, C.c_void_p(a["y"]) if a["y"] else None, a["B"],
                                a["T"], a["C"], a["sb"], a["st"], a["sc"], None if ln is None else C.c_void_p(ln.ctypes.data),
                                C.c_void_p(a["ws"]) if a["ws"] else None, a["nb"])

    def refused(code, want, *words):
        msg = lib.dfa_last_error(h).decode()
        assert code == want, (code, want, msg)
        assert msg.strip(), "a refusal without a message"
        for w in words:
            assert w in msg, (w, msg)

    assert call(h=None) == _lib.E_NULL_PTR
    for name in ("x", "y", "ws"):
        refused(call(**{name: None}), _lib.E_NULL_PTR, "non-null")
    for mode in (0, 3, -1):
        refused(call(mode=mode), _lib.E_UNSUPPORTED, "mode")
    refused(call(B=0), _lib.E_BAD_SHAPE, "batch")
    refused(call(C=0), _lib.E_BAD_SHAPE, "C must be")
    refused(call(T=0), _lib.E_BAD_SHAPE, "T_max")
    refused(call(ln=[10, 0, 2]), _lib.E_BAD_SHAPE, "lengths[1]=0")
    refused(call(ln=[10, 7, 11]), _lib.E_BAD_SHAPE, "lengths[2]=11")
    refused(call(ln=[10, 1, 2]), _lib.E_BAD_SHAPE, "lengths[1]=1", "cvmn")
    refused(call(ln=None, T=1, mode=2), _lib.E_BAD_SHAPE, "cvmn")
    refused(call(st=2, sc=3), _lib.E_UNSUPPORTED, "stride_t", "stride_c")
    refused(call(x=xs.data_ptr() + 4), _lib.E_UNSUPPORTED, "16-byte")          # misaligned base
    refused(call(y=ys.data_ptr() + 8), _lib.E_UNSUPPORTED, "16-byte")
    refused(call(sc=P + 1), _lib.E_UNSUPPORTED, "stride_c")                     # misaligned pitch
    refused(call(sc=8), _lib.E_UNSUPPORTED, "stride_c")                         # rows shorter than T_max
    refused(call(sb=Cc * P + 2), _lib.E_UNSUPPORTED, "stride_b")
    refused(call(st=Cc - 1, sc=1), _lib.E_UNSUPPORTED, "stride_t")             # feature fastest: frames overlap
    refused(call(nb=need - 1), _lib.E_WORKSPACE, "workspace")
    refused(call(ws=ws.data_ptr() + 16), _lib.E_WORKSPACE, "aligned")
    # the packed form
    off = np.array([0, Cc * P], dtype=np.int64)

    def packed(**kw):
        a = dict(mode=2, set=ys.data_ptr(), n=ys.numel(), off=off, ln=[10, 9], N=2, C=Cc, ws=ws.data_ptr(), nb=need)
        a.update(kw)
        o, ln = np.asarray(a["off"], dtype=np.int64), np.asarray(a["ln"], dtype=np.int32)
        return lib.dfa_utt_norm_packed(h, a["mode"], C.c_void_p(a["set"]) if a["set"] else None, a["n"], C.c_void_p(o.ctypes.data),
                                       C.c_void_p(ln.ctypes.data), a["N"], a["C"], C.c_void_p(a["ws"]), a["nb"])

    refused(packed(set=None), _lib.E_NULL_PTR, "non-null")
    refused(packed(mode=5), _lib.E_UNSUPPORTED, "mode")
    refused(packed(N=0), _lib.E_BAD_SHAPE, "N must be")
    refused(packed(N=_lib.UTT_NORM_MAX_PACKED + 1), _lib.E_UNSUPPORTED, "chunks")
    refused(packed(ln=[10, 1]), _lib.E_BAD_SHAPE, "lengths[1]=1")
    refused(packed(ln=[0, 9]), _lib.E_BAD_SHAPE, "lengths[0]=0")
    refused(packed(off=[0, 46]), _lib.E_BAD_SHAPE, "offsets[1]=46")
    refused(packed(off=[0, -4]), _lib.E_BAD_SHAPE, "offsets[1]=-4")
    refused(packed(n=Cc * P + Cc * P - 1), _lib.E_BAD_SHAPE, "offsets[1]")
    refused(packed(set=ys.data_ptr() + 4), _lib.E_UNSUPPORTED, "16-byte")
    refused(packed(nb=8), _lib.E_WORKSPACE, "workspace")
    # a capturing stream: the lengths are per-call data
    for entry in (call, packed):
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with pytest.raises(ValueError, match="captured"):
            with torch.cuda.graph(graph):
                ctx.use_current_stream()
                _lib.check(h, entry())
    ctx.use_current_stream()
    torch.cuda.synchronize()
    assert bool((ys == 7.0).all())                                     # nothing was written by any refused call
    assert call() == 0 and packed(mode=1, set=xs.data_ptr(), n=xs.numel()) == 0          # and the context still works
    torch.cuda.synchronize()
    assert bool(torch.isfinite(ys[:B * Cc * P]).all()) and not bool((ys[:B * Cc * P] == 7.0).all())


# 6 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", UO.MODES)
def test_resident_batcher_holds_the_normalised_set(mode):
    from dfa_amd.dataloaders import ResidentBatcher
    from dfa_amd.normalization import normalize_batch
    g = torch.Generator().manual_seed(6)
    feats = torch.randn(11, 8, 37, generator=g) * 3.0 + torch.arange(8.0).view(1, 8, 1)
    labels = (torch.arange(11) % 2).float()
    idx = torch.tensor([10, 3, 3, 0, 7, 9, 1, 5])
    raw = list(ResidentBatcher(feats, labels, 3, device="cuda").epoch(idx))
    res = ResidentBatcher(feats, labels, 3, device="cuda", chunk_rows=4, norm=mode)
    got = list(res.epoch(idx))
    assert len(got) == len(raw) == 3 and res.features.dtype == torch.float32
    for (f, l), (fr, lr) in zip(got, raw):
        want = normalize_batch(fr.transpose(1, 2), mode).transpose(1, 2)
        assert f.shape == fr.shape and torch.equal(l, lr)
        assert np.array_equal(_bits(f), _bits(want))
        y64 = UO.normalize(fr[0].cpu().numpy(), mode)                  # and it is the normalisation
        assert (np.abs(f[0].cpu().numpy() - y64).max(axis=1) <= UO.row_bound(fr[0].cpu().numpy(), mode)).all()
    # bf16 storage: normalised in float32 first, rounded afterwards
    res16 = ResidentBatcher(feats, labels, 3, device="cuda", dtype=torch.bfloat16, norm=mode)
    assert torch.equal(res16.features, res.features.to(torch.bfloat16))
    assert torch.equal(ResidentBatcher(feats, None, 3, device="cuda", norm="raw").features.cpu(), feats)


# 7 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", UO.MODES)
def test_dlq_resident_set_normalises_then_masks(mode):
    from dfa_amd.dataloaders import DlqResidentSet
    from dfa_amd.normalization import normalize_batch
    Cc = 12
    lens = [9, 65, 2, 130, 33, 257]
    feats = [torch.from_numpy(np.array(UO.utterance(Cc, T, seed=7))) for T in lens]
    raw = DlqResidentSet(feats, None, device="cuda")
    nset = DlqResidentSet(feats, None, device="cuda", chunk_utts=4, norm=mode)
    assert nset.norm == mode and raw.norm == "raw"
    idx = [3, 0, 5, 5, 2]
    spans = np.array([[[100, 20], [0, 5], [2, 3]], [[0, 0], [8, 1], [0, 12]], [[250, 7], [3, 30], [11, 1]], [[0, 257], [0, 0], [0, 0]],
                      [[1, 1], [0, 0], [5, 2]]], dtype=np.int32)
    x, lengths, _ = raw.batch(idx)
    want = normalize_batch(x.transpose(1, 2), mode, lengths).transpose(1, 2).clone()
    plain, lengths_n, _ = nset.batch(idx)
    assert np.array_equal(lengths, lengths_n) and np.array_equal(_bits(plain), _bits(want))
    for j, sp in enumerate(spans.tolist()):
        for k, (s0, w) in enumerate(sp):
            if k < 2:
                want[j, :, s0:s0 + w] = 0.0
            else:
                want[j, s0:s0 + w, :] = 0.0
    masked, _, _ = nset.batch(idx, spans, 2)
    assert np.array_equal(_bits(masked), _bits(want))


# 8 ------------------------------------------------------------------------------------------------------------------------------
def test_predict_scores_ragged_normalises_each_utterance(golden):
    from dfa_amd.model_cnn1d import CNN1D
    from dfa_amd.normalization import normalize_batch
    from dfa_amd.predict import predict_scores, predict_scores_ragged
    torch.manual_seed(3)
    model = CNN1D(in_features=180, dropout=0.2).to("cuda").eval()
    lens = [321, 40, 257, 64, 9]
    utts = [torch.from_numpy(np.array(UO.utterance(180, T, seed=8))) for T in lens]
    got = predict_scores_ragged(model, utts, batch_size=3, device="cuda", apply_sigmoid=False, norm="cvmn")
    raw = predict_scores_ragged(model, utts, batch_size=3, device="cuda", apply_sigmoid=False)
    with torch.no_grad():
        for i, u in enumerate(utts):
            x, ln = _batch([u.numpy()], "time", behind=0.0)
            alone = model(normalize_batch(x, "cvmn", ln), lengths=ln).squeeze(-1)
            assert torch.equal(alone, got[i:i + 1]), lens[i]
    assert not torch.equal(raw, got)
    # the stacked path: each batch is normalised where it reaches the device
    same = torch.stack([torch.from_numpy(np.array(UO.utterance(180, 321, seed=s))) for s in range(4)])
    a = predict_scores(model, same, batch_size=3, device="cuda", apply_sigmoid=False, norm="cmn")
    with torch.no_grad():
        b = torch.cat([model(normalize_batch(same[lo:lo + 3].to("cuda").transpose(1, 2), "cmn")).squeeze(-1) for lo in (0, 3)])
    assert torch.equal(a, b) and not torch.equal(a, predict_scores(model, same, batch_size=3, device="cuda", apply_sigmoid=False))
