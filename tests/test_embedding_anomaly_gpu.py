"""GPU side of the embedding anomaly detectors (dfa_emb_* of include/dfa_hip.h, dfa_amd/embedding_anomaly.py), through ctypes
and without sklearn (but the command-line test).  The oracle of every parity test is the float64 numpy statement of the scores
from the fitted arrays (tests/emb_oracle.py); the same statement in float32 numpy gives e32, and the GPU must stay within
4 * max(e32, 2^-22) with e = max|s - s64| / max|s64|.

Measured on an MI355X, the worst case of each family as e_gpu / e32 (the smallest bound is 4 * 2^-22 = 9.5e-7):
    D = 128:    OC-SVM 3.1e-7 / 3.9e-7 (n_sv = 1: 1.9e-6 / 1.9e-6, bound 7.7e-6)   GMM 8.6e-8 / 8.3e-8
    D = 640:    OC-SVM 3.7e-7 / 4.1e-7                                              GMM 8.8e-8 / 8.5e-8
    D = 23040:  OC-SVM 1.5e-7 / 2.1e-7                                              GMM 1.5e-7 / 7.0e-8
    fixture:    OC-SVM 1.7e-7 / 2.4e-7                                              GMM 6.2e-8 / 8.4e-8"""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

import emb_oracle as EO
import workspace_bands as WB

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DET_KEYS = ("mean", "inv_scale", "sv", "dual_coef", "gamma", "intercept", "pca_mean", "components", "means", "prec_chol", "log_const")
PATTERNS = [0xFFFF, 0x7FC0, 0x7F80]                     # as tests/test_lds_poison_gpu.py


def _lib():
    from dfa_amd import _lib
    return _lib


def _ctx():
    return _lib().Context.get(torch.device("cuda"))


@pytest.fixture(scope="module")
def fx():
    with np.load(os.path.join(ROOT, "tests", "golden", "emb_detectors.npz")) as z:
        return {k: z[k] for k in z.files}


class Raw:
    """One detector pair bound through the C ABI: the arrays as device tensors, the two calls on an explicit workspace."""

    def __init__(self, det):
        L = _lib()
        self.L, self.ctx = L, _ctx()
        self.det = det
        self.t = {k: torch.from_numpy(np.asarray(det[k], dtype=np.float32)).cuda() for k in DET_KEYS if k not in ("gamma", "intercept")}
        self.D, self.n_sv = det["sv"].shape[1], det["sv"].shape[0]
        self.P, self.K = det["components"].shape[0], det["means"].shape[0]
        self.bind()

    def bind(self):
        L, t, h = self.L, self.t, self.ctx.handle
        self.ctx.use_current_stream()
        p = L.ptr
        L.check(h, self.ctx.lib.dfa_emb_ocsvm_bind(h, self.D, self.n_sv, p(t["mean"]), p(t["inv_scale"]), p(t["sv"]), p(t["dual_coef"]),
                                                   float(self.det["gamma"]), float(self.det["intercept"])))
        L.check(h, self.ctx.lib.dfa_emb_gmm_bind(h, self.D, self.P, self.K, p(t["mean"]), p(t["inv_scale"]), p(t["pca_mean"]), p(t["components"]),
                                                 p(t["means"]), p(t["prec_chol"]), p(t["log_const"])))

    def nbytes(self, which, N):
        lib = self.ctx.lib
        return lib.dfa_emb_workspace_bytes(self.L.EMB_OCSVM, N, self.D, self.n_sv, 0) if which == "ocsvm" else \
            lib.dfa_emb_workspace_bytes(self.L.EMB_GMM, N, self.D, self.P, self.K)

    def call(self, which, emb, out, ws, ws_bytes=None, stride=None, N=None, D=None):
        """the raw return code"""
        fn = self.ctx.lib.dfa_emb_ocsvm_score if which == "ocsvm" else self.ctx.lib.dfa_emb_gmm_score
        self.ctx.use_current_stream()
        return fn(self.ctx.handle, self.L.ptr(emb), emb.shape[0] if N is None else N, self.D if D is None else D,
                  emb.stride(0) if stride is None else stride, self.L.ptr(out), self.L.ptr(ws), ws.numel() if ws_bytes is None else ws_bytes)

    def score(self, which, emb, ws=None):
        """device [n, D] float32 rows (any row stride) -> host float32 [n]"""
        N = emb.shape[0]
        if ws is None:
            ws = torch.full((self.nbytes(which, N),), 0xFF, dtype=torch.uint8, device="cuda")      # exact size, NaN bytes
        out = torch.full((N,), float("nan"), dtype=torch.float32, device="cuda")
        self.L.check(self.ctx.handle, self.call(which, emb, out, ws, stride=max(emb.stride(0), self.D)))
        return out.cpu().numpy()


def _strided(x, extra):
    """host [n, D] -> device rows `D + extra` floats apart, NaN between them"""
    n, D = x.shape
    buf = torch.full((n, D + extra), float("nan"), dtype=torch.float32, device="cuda")
    buf[:, :D] = torch.from_numpy(x).cuda()
    return buf[:, :D]


def _check(which, got, det, x, what):
    s64, e32, tol = EO.bound(det, x, which)
    e = EO.rel_err(got, s64)
    print(f"{what} {which}: e_gpu = {e:.3e}  e32 = {e32:.3e}  allowed = {tol:.3e}  max|s64| = {np.abs(s64).max():.4g}")
    assert np.isfinite(got).all(), what
    assert e <= tol, f"{what} {which}: e_gpu {e:.3e} > 4 * max(e32 {e32:.3e}, 2^-22) = {tol:.3e}"


# (D, N, n_sv, P, K, extra row stride): every value of the issue's lists once, each edge with a neighbour of another kind
CASES = [
    (128, 1, 1, 1, 1, 0),
    (128, 2, 33, 7, 3, 0),
    (128, 63, 70, 33, 8, 128),
    (128, 65, 257, 128, 1, 0),
    (640, 65, 257, 256, 3, 0),
    (640, 130, 70, 33, 1, 128),
    (640, 130, 257, 7, 8, 0),
    (640, 2, 1, 256, 8, 128),
    (23040, 3, 40, 256, 8, 0),        # the real D: every split of the long reduction
]


@pytest.mark.parametrize("D,N,n_sv,P,K,extra", CASES)
def test_parity_against_the_float64_statement(D, N, n_sv, P, K, extra):
    det, rows = EO.random_detectors(1000 + D + N + n_sv + P + K, D, n_sv, P, K)
    x = rows(N)
    raw = Raw(det)
    emb = _strided(x, extra)
    assert emb.stride(0) == D + extra
    for which in ("ocsvm", "gmm"):
        _check(which, raw.score(which, emb), det, x, f"D={D} N={N} n_sv={n_sv} P={P} K={K} stride={D + extra}")


def test_fixture_parity_and_eer(fx):
    raw = Raw(fx)
    from dfa_amd.evaluation import calculate_eer
    emb = torch.from_numpy(fx["dev"]).cuda()
    for which, fn in (("ocsvm", EO.ocsvm_scores), ("gmm", EO.gmm_scores)):
        got = raw.score(which, emb)
        _check(which, got, fx, fx["dev"], "fixture")
        want = calculate_eer(fn(fx, fx["dev"]).tolist(), fx["labels"].tolist())
        have = calculate_eer(got.astype(np.float64).tolist(), fx["labels"].tolist())
        assert have[0] == want[0] and 0.0 < have[0] < 0.5, (which, have, want)


def test_a_row_scores_the_same_alone_in_a_pair_and_in_a_batch_of_130():
    det, rows = EO.random_detectors(77, 640, 257, 33, 8)
    x = rows(130)
    raw = Raw(det)
    emb = torch.from_numpy(x).cuda()
    for which in ("ocsvm", "gmm"):
        full = raw.score(which, emb)
        assert raw.score(which, emb).tobytes() == full.tobytes(), f"{which}: two runs of the same call differ"
        for i in (0, 1, 31, 32, 63, 64, 127, 128, 129):
            alone = raw.score(which, emb[i:i + 1].clone())
            pair = raw.score(which, torch.stack([emb[i], emb[(i + 57) % 130]]))
            assert alone.tobytes() == full[i:i + 1].tobytes(), f"{which}: row {i} alone differs from row {i} of the batch"
            assert pair[:1].tobytes() == full[i:i + 1].tobytes(), f"{which}: row {i} as row 0 of a pair differs from the batch"


def test_real_width_rows_are_independent_too():
    det, rows = EO.random_detectors(78, 23040, 40, 256, 8)
    x = rows(3)
    raw = Raw(det)
    emb = torch.from_numpy(x).cuda()
    for which in ("ocsvm", "gmm"):
        full = raw.score(which, emb)
        assert raw.score(which, emb[2:3].clone()).tobytes() == full[2:3].tobytes(), which


def test_poisoned_lds_and_nan_workspace_change_no_bit(fx):
    raw = Raw(fx)
    emb = torch.from_numpy(fx["dev"]).cuda()
    for which in ("ocsvm", "gmm"):
        ws = torch.zeros(raw.nbytes(which, 100) + 4096, dtype=torch.uint8, device="cuda")
        clean = raw.score(which, emb, ws)
        for pat in PATTERNS:
            raw.ctx.set_option("poison_lds", pat)
            ws.fill_(0xFF)
            assert raw.score(which, emb, ws).tobytes() == clean.tobytes(), f"{which}: poison_lds {pat:#x} + NaN workspace"


@pytest.mark.parametrize("N", [1, 100])
def test_exact_size_workspace_between_canary_bands(fx, N):
    raw = Raw(fx)
    emb = torch.from_numpy(fx["dev"][:N]).cuda()
    for which in ("ocsvm", "gmm"):
        nbytes = raw.nbytes(which, N)
        assert nbytes > 0 and nbytes % 256 == 0
        want = raw.score(which, emb, WB.roomy(nbytes))
        view, check = WB.banded(nbytes)
        got = raw.score(which, emb, view)
        check(f"{which} N={N}")
        assert got.tobytes() == want.tobytes(), which
        # one byte short: refused, nothing written
        view, check = WB.banded(nbytes)
        out = torch.full((N,), 7.0, dtype=torch.float32, device="cuda")
        code = raw.call(which, emb, out, view, ws_bytes=nbytes - 1)
        assert code == raw.L.E_WORKSPACE and "workspace too small" in raw.ctx.lib.dfa_last_error(raw.ctx.handle).decode()
        check(f"{which} N={N}, refused")
        assert bool((out == 7.0).all()) and bool((view == 0xFF).all())


def test_refusals_name_the_argument(fx):
    L = _lib()
    raw = Raw(fx)
    ctx, lib, t = raw.ctx, raw.ctx.lib, raw.t
    h, p = ctx.handle, L.ptr

    def err():
        return lib.dfa_last_error(h).decode()

    def bind_svm(D=640, n_sv=None, **null):
        a = {k: p(t[k]) for k in ("mean", "inv_scale", "sv", "dual_coef")}
        a.update(null)
        return lib.dfa_emb_ocsvm_bind(h, D, raw.n_sv if n_sv is None else n_sv, a["mean"], a["inv_scale"], a["sv"], a["dual_coef"],
                                      float(fx["gamma"]), float(fx["intercept"]))

    def bind_gmm(D=640, P=32, K=4, **null):
        a = {k: p(t[k]) for k in ("mean", "inv_scale", "pca_mean", "components", "means", "prec_chol", "log_const")}
        a.update(null)
        return lib.dfa_emb_gmm_bind(h, D, P, K, a["mean"], a["inv_scale"], a["pca_mean"], a["components"], a["means"], a["prec_chol"],
                                    a["log_const"])

    emb = torch.from_numpy(fx["dev"][:4]).cuda()
    out = torch.zeros(4, dtype=torch.float32, device="cuda")
    ws = torch.zeros(max(raw.nbytes("ocsvm", 4), raw.nbytes("gmm", 4)) + 256, dtype=torch.uint8, device="cuda")
    for fn, kw, want, word in ((bind_svm, {"D": 100}, L.E_BAD_SHAPE, "D=100"), (bind_gmm, {"D": 100}, L.E_BAD_SHAPE, "D=100"),
                               (bind_svm, {"D": 0}, L.E_BAD_SHAPE, "D=0"), (bind_gmm, {"D": -128}, L.E_BAD_SHAPE, "D=-128"),
                               (bind_gmm, {"P": 0}, L.E_BAD_SHAPE, "P=0"), (bind_gmm, {"P": 257}, L.E_BAD_SHAPE, "P=257"),
                               (bind_gmm, {"K": 0}, L.E_BAD_SHAPE, "K=0"), (bind_gmm, {"K": 65}, L.E_BAD_SHAPE, "K=65"),
                               (bind_svm, {"n_sv": 0}, L.E_BAD_SHAPE, "n_sv=0"),
                               (bind_svm, {"sv": None}, L.E_NULL_PTR, "sv"), (bind_svm, {"dual_coef": None}, L.E_NULL_PTR, "dual_coef"),
                               (bind_svm, {"mean": None}, L.E_NULL_PTR, "mean"), (bind_gmm, {"inv_scale": None}, L.E_NULL_PTR, "inv_scale"),
                               (bind_gmm, {"pca_mean": None}, L.E_NULL_PTR, "pca_mean"), (bind_gmm, {"components": None}, L.E_NULL_PTR, "components"),
                               (bind_gmm, {"means": None}, L.E_NULL_PTR, "means"), (bind_gmm, {"prec_chol": None}, L.E_NULL_PTR, "prec_chol"),
                               (bind_gmm, {"log_const": None}, L.E_NULL_PTR, "log_const")):
        code = fn(**kw)
        assert code == want and word in err(), (kw, code, err())
        # a refused bind leaves that detector unbound
        which = "ocsvm" if fn is bind_svm else "gmm"
        assert raw.call(which, emb, out, ws) == L.E_NOT_PREPARED and "bind" in err()
        raw.bind()
    for which in ("ocsvm", "gmm"):
        assert raw.call(which, emb, out, ws, stride=639) == L.E_BAD_SHAPE and "stride_n" in err()
        assert raw.call(which, emb, out, ws, stride=642) == L.E_UNSUPPORTED and "stride_n" in err()
        assert raw.call(which, emb, out, ws, N=0) == L.E_BAD_SHAPE and "N=0" in err()
        assert raw.call(which, emb, out, ws, D=100) == L.E_BAD_SHAPE and "D=100" in err()
        assert raw.call(which, emb, out, ws, D=128) == L.E_BAD_SHAPE and "D=128" in err()
        fn = lib.dfa_emb_ocsvm_score if which == "ocsvm" else lib.dfa_emb_gmm_score
        assert fn(h, None, 4, 640, 640, p(out), p(ws), ws.numel()) == L.E_NULL_PTR and "emb" in err()
        assert fn(h, p(emb), 4, 640, 640, None, p(ws), ws.numel()) == L.E_NULL_PTR and "out" in err()
        assert fn(h, p(emb), 4, 640, 640, p(out), None, ws.numel()) == L.E_NULL_PTR and "workspace" in err()
        assert fn(None, p(emb), 4, 640, 640, p(out), p(ws), ws.numel()) == L.E_NULL_PTR
        assert fn(h, p(emb), 4, 640, 640, p(out), C.c_void_p(ws.data_ptr() + 64), ws.numel() - 64) == L.E_WORKSPACE and "aligned" in err()
    torch.cuda.synchronize()
    assert bool((out == 0).all())                     # no refused call wrote a score
    _check("ocsvm", raw.score("ocsvm", emb), fx, fx["dev"][:4], "after the refusals")


def _small_model():
    from dfa_amd.model import CNN2D
    torch.manual_seed(11)
    model = CNN2D(in_features=5, dropout=0.0).to("cuda").eval()
    with torch.no_grad():
        for i in (1, 6, 11):
            model.conv[i].running_mean.normal_(0.0, 0.2)
            model.conv[i].running_var.uniform_(0.5, 1.5)
    return model


def test_end_to_end_scores_stay_on_the_device(fx):
    from dfa_amd import embedding_anomaly as EA
    det = EA.Detectors(**{k: fx[k] for k in DET_KEYS})
    scorer = EA.EmbeddingScorer(det, "cuda")
    model = _small_model()
    x = torch.randn(4, 24, 5, generator=torch.Generator().manual_seed(12)).cuda()
    logits, s_svm, s_gmm = scorer.score_features(model, x)
    with torch.no_grad():
        logits2, emb = model(x, return_embedding=True)
    assert emb.shape == (4, 640) and s_svm.device.type == "cuda" and s_gmm.shape == (4,)
    assert torch.equal(logits, logits2)
    assert torch.equal(s_svm, scorer.ocsvm_scores(emb)) and torch.equal(s_gmm, scorer.gmm_scores(emb))
    e = emb.cpu().numpy()
    _check("ocsvm", s_svm.cpu().numpy(), fx, e, "CNN2D(in_features=5) embedding")
    _check("gmm", s_gmm.cpu().numpy(), fx, e, "CNN2D(in_features=5) embedding")
    # a second scorer takes the context's slots; the first binds again when it is used next
    d2, rows = EO.random_detectors(5, 640, 33, 7, 3)
    other = EA.EmbeddingScorer(EA.Detectors(**{k: d2[k] for k in DET_KEYS}), "cuda")
    _check("gmm", other.gmm_scores(emb).cpu().numpy(), d2, e, "second scorer")
    assert torch.equal(scorer.gmm_scores(emb), s_gmm) and torch.equal(scorer.ocsvm_scores(emb), s_svm)
    # strided rows, and the fixture's dev set through the module: the same EER as the float64 scores
    wide = torch.zeros(4, 768, device="cuda")
    wide[:, :640] = emb
    assert torch.equal(scorer.ocsvm_scores(wide[:, :640]), s_svm)
    from dfa_amd.evaluation import calculate_eer
    dev = torch.from_numpy(fx["dev"]).cuda()
    for got, fn in ((scorer.ocsvm_scores(dev), EO.ocsvm_scores), (scorer.gmm_scores(dev), EO.gmm_scores)):
        want = calculate_eer(fn(fx, fx["dev"]).tolist(), fx["labels"].tolist())
        assert calculate_eer(got.double().cpu().tolist(), fx["labels"].tolist())[0] == want[0]
    with pytest.raises(ValueError, match="D=128"):
        scorer.ocsvm_scores(torch.zeros(2, 128, device="cuda"))
    with pytest.raises(RuntimeError, match="device tensors"):
        scorer.gmm_scores(torch.zeros(2, 640))


def test_cli_fits_scores_saves_and_rescoring_needs_no_sklearn(tmp_path, capsys, monkeypatch):
    pytest.importorskip("sklearn")
    import pandas as pd
    from dfa_amd import embedding_anomaly as EA
    model = _small_model()
    ckpt = str(tmp_path / "cnn2d.pt")
    torch.save({"model_state": model.state_dict()}, ckpt)
    g = torch.Generator().manual_seed(13)
    paths = {}
    for split in ("train", "dev"):
        ids = [f"{split}{i:03d}" for i in range(64)]
        labels = [1 if i % 4 else 0 for i in range(64)]
        feats = [torch.randn(5, 24, generator=g) * (1.0 if l else 1.6) + (0.0 if l else 0.3) for l in labels]
        pd.DataFrame({"uttid": ids, "features": feats}).to_pickle(str(tmp_path / f"{split}_features.pkl"))
        pd.DataFrame({"uttid": ids, "label": labels}).to_pickle(str(tmp_path / f"{split}_labels.pkl"))
        paths[split] = (str(tmp_path / f"{split}_features.pkl"), str(tmp_path / f"{split}_labels.pkl"))
    common = ["--checkpoint", ckpt, "--train-features", paths["train"][0], "--train-labels", paths["train"][1], "--dev-features", paths["dev"][0],
              "--dev-labels", paths["dev"][1], "--in-features", "5", "--dropout", "0.0", "--gmm-components", "2"]
    det_path, out_path = str(tmp_path / "det.npz"), str(tmp_path / "prediction.pkl")
    first = EA.main(common + ["--save-detectors", det_path])
    text = capsys.readouterr().out
    assert "One-Class SVM  EER = " in text and "GMM            EER = " in text and "threshold = " in text
    assert "Embedding Anomaly Detection Results (dev set)" in text and "Bonafide training embeddings: (48, 640)" in text
    assert first["ocsvm"].shape == (64,) and np.isfinite(first["ocsvm"]).all() and np.isfinite(first["gmm"]).all()
    monkeypatch.setitem(sys.modules, "sklearn", None)          # any import of sklearn now raises
    again = EA.main(common + ["--detectors", det_path, "--out", out_path, "--score", "gmm"])
    assert again["ocsvm"].tobytes() == first["ocsvm"].tobytes() and again["gmm"].tobytes() == first["gmm"].tobytes()
    pred = pd.read_pickle(out_path)
    assert list(pred.columns) == ["uttid", "predictions"] and list(pred["uttid"]) == [f"dev{i:03d}" for i in range(64)]
    assert pred["predictions"].to_numpy().tobytes() == first["gmm"].tobytes()
