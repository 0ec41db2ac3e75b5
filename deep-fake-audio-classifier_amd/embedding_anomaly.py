"""Anomaly detection on CNN2D embeddings -- counterpart of src/embedding_anomaly.py (same arguments, defaults and result lines).

The trained CNN2D is the feature extractor; a StandardScaler, a One-Class SVM and a PCA + full-covariance GMM are fitted on the
bonafide training embeddings with sklearn on the host (a one-off, as in the reference: `fit_detectors`), and the dev set is scored
by its distance from that "normal" distribution.  The scoring runs where the embeddings already are: `EmbeddingScorer` binds the
fitted arrays to the device (dfa_emb_ocsvm_bind / dfa_emb_gmm_bind) and scores the forward's embedding rows in place
(dfa_emb_ocsvm_score / dfa_emb_gmm_score), so a batch sends its scores to the host, not its 92 KB-per-utterance embeddings.
A fitted `Detectors` record is plain arrays (`.save` / `.load`: an .npz); scoring needs no sklearn.  There is no CPU path.

    python -m dfa_amd.embedding_anomaly --checkpoint cnn2d_best.pt [--save-detectors det.npz]
    python -m dfa_amd.embedding_anomaly --checkpoint cnn2d_best.pt --detectors det.npz --out prediction.pkl --score ocsvm
"""
from __future__ import annotations

import argparse
import dataclasses

import numpy as np
import torch

from . import _lib
from .evaluation import calculate_eer
from .model import CNN2D

_FIELDS = ("mean", "inv_scale", "sv", "dual_coef", "gamma", "intercept", "pca_mean", "components", "means", "prec_chol",
           "log_const")


def resolve_device(device_arg):
    """src/embedding_anomaly.py:26-33, on a machine whose only path is the GPU."""
    return device_arg or "cuda"


def load_model(checkpoint_path: str, device: str, in_features: int = 180, dropout: float = 0.2, precision: str = "fp32") -> CNN2D:
    """src/embedding_anomaly.py:36-46: the reference's checkpoint dict {"model_state": ...} or a bare state_dict."""
    from .predict import load_weights
    model = CNN2D(in_features=in_features, dropout=dropout, precision=precision).to(device)
    load_weights(model, checkpoint_path, device)
    return model.eval()


def _source(features):
    """A stacked [N, F, T] tensor stays one; a sequence of per-utterance [F, T_i] tensors is stacked when the lengths agree and
    stays a list (the ragged source of dataloaders.EvalBatches) when they do not."""
    if isinstance(features, torch.Tensor):
        return features
    feats = [f.float() for f in features]
    if len({tuple(f.shape) for f in feats}) > 1:
        return feats
    return torch.stack(feats)


def _check_ragged(model, source, swap_tf):
    if isinstance(source, list):
        from .predict import check_ragged_args
        check_ragged_args("cnn2d", model.precision, swap_tf)


@torch.no_grad()
def extract_embeddings(model: CNN2D, features, labels, batch_size: int = 32, device="cuda", swap_tf: bool = True,
                       bonafide_only: bool = False, input_dtype=None):
    """src/embedding_anomaly.py:49-73 on the HIP forward (predict._forward_batches, uniform or ragged): (embeddings [n, 128 F],
    labels [n]) as host float32 arrays in input order -- the rows with label 1 alone when bonafide_only.  For the fit."""
    from .predict import _forward_batches
    source = _source(features)
    _check_ragged(model, source, swap_tf)
    labels = np.asarray(labels, dtype=np.float32).reshape(-1)
    if len(source) != labels.shape[0]:
        raise ValueError(f"{len(source)} utterances but {labels.shape[0]} labels")
    _, emb = _forward_batches(model, source, batch_size, device, 0, 1, input_dtype, swap_tf, return_embedding=True)
    emb = np.zeros((0, 0), np.float32) if emb is None else emb.numpy()
    if bonafide_only:
        mask = labels == 1.0
        emb, labels = emb[mask], labels[mask]
    return emb, labels


@dataclasses.dataclass
class Detectors:
    """A fitted scaler + One-Class SVM + PCA + GMM as float32 arrays (include/dfa_hip.h has the formulas):
    mean[D], inv_scale[D]; sv[n_sv][D], dual_coef[n_sv], gamma, intercept; pca_mean[D], components[P][D], means[K][P],
    prec_chol[K][P][P], log_const[K]."""
    mean: np.ndarray
    inv_scale: np.ndarray
    sv: np.ndarray
    dual_coef: np.ndarray
    gamma: np.ndarray
    intercept: np.ndarray
    pca_mean: np.ndarray
    components: np.ndarray
    means: np.ndarray
    prec_chol: np.ndarray
    log_const: np.ndarray

    def __post_init__(self):
        for name in _FIELDS:
            setattr(self, name, np.require(getattr(self, name), dtype=np.float32, requirements="C"))
        D, P, K = self.mean.shape[0], self.components.shape[0], self.means.shape[0]
        want = {"mean": (D,), "inv_scale": (D,), "sv": (self.sv.shape[0], D), "dual_coef": (self.sv.shape[0],), "gamma": (),
                "intercept": (), "pca_mean": (D,), "components": (P, D), "means": (K, P), "prec_chol": (K, P, P), "log_const": (K,)}
        for name, shape in want.items():
            if getattr(self, name).shape != shape:
                raise ValueError(f"Detectors.{name} has shape {getattr(self, name).shape}, expected {shape}")

    def __getitem__(self, name):
        if name not in _FIELDS:
            raise KeyError(name)
        return getattr(self, name)

    @property
    def dims(self):
        """(D, n_sv, P, K)"""
        return self.mean.shape[0], self.sv.shape[0], self.components.shape[0], self.means.shape[0]

    def save(self, path: str) -> None:
        with open(path, "wb") as fh:
            np.savez(fh, **{name: getattr(self, name) for name in _FIELDS})

    @classmethod
    def load(cls, path: str) -> "Detectors":
        with np.load(path, allow_pickle=False) as z:
            missing = [name for name in _FIELDS if name not in z.files]
            if missing:
                raise ValueError(f"{path} is not a Detectors file: it lacks {missing}")
            return cls(**{name: z[name] for name in _FIELDS})


def fit_detectors(train_emb, gmm_components: int = 8, svm_nu: float = 0.05, svm_kernel: str = "rbf") -> Detectors:
    """src/embedding_anomaly.py:129-158 on the host: StandardScaler -> OneClassSVM(rbf, nu) -> PCA(min(256, D, N),
    random_state=42) -> GaussianMixture(full, reg_covar=1e-4, random_state=42), returned as arrays.  gamma is resolved as
    sklearn's 'scale': 1 / (D * var of the scaled training matrix)."""
    if svm_kernel != "rbf":
        raise ValueError(f"--svm-kernel {svm_kernel!r} is not supported: the GPU scorer implements the reference's default, "
                         "'rbf', alone, and there is no CPU fallback")
    from sklearn.decomposition import PCA
    from sklearn.mixture import GaussianMixture
    from sklearn.preprocessing import StandardScaler
    from sklearn.svm import OneClassSVM

    train_emb = np.asarray(train_emb)
    if train_emb.ndim != 2 or train_emb.shape[0] < 2:
        raise ValueError(f"fit_detectors needs a [n >= 2, D] matrix of training embeddings, got shape {train_emb.shape}")
    scaler = StandardScaler()
    xs = scaler.fit_transform(train_emb)
    ocsvm = OneClassSVM(kernel="rbf", nu=svm_nu).fit(xs)
    var = float(np.asarray(xs, dtype=np.float64).var())      # (the SVM is fitted on the float64 copy of its input)
    gamma = 1.0 / (xs.shape[1] * var) if var != 0 else 1.0
    n_pca = min(256, xs.shape[1], xs.shape[0])
    pca = PCA(n_components=n_pca, random_state=42)
    train_pca = pca.fit_transform(xs)
    gmm = GaussianMixture(n_components=gmm_components, covariance_type="full", reg_covar=1e-4, random_state=42).fit(train_pca)
    chol = np.asarray(gmm.precisions_cholesky_, dtype=np.float64)
    log_det = np.log(np.diagonal(chol, axis1=1, axis2=2)).sum(axis=1)
    log_const = log_det + np.log(gmm.weights_) - 0.5 * n_pca * np.log(2.0 * np.pi)
    return Detectors(mean=scaler.mean_, inv_scale=1.0 / scaler.scale_, sv=ocsvm.support_vectors_, dual_coef=ocsvm.dual_coef_[0],
                     gamma=gamma, intercept=ocsvm.intercept_[0], pca_mean=pca.mean_, components=pca.components_,
                     means=gmm.means_, prec_chol=chol, log_const=log_const)


class EmbeddingScorer:
    """`detectors` on `device`: the arrays as device tensors, bound to the device's context on first use and again whenever
    another scorer used the context's detector slots in between."""

    def __init__(self, detectors: Detectors, device="cuda"):
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError(f"dfa_amd.EmbeddingScorer runs on the GPU only (got device '{device}'); there is no CPU path")
        self.detectors = detectors
        self.D, self.n_sv, self.P, self.K = detectors.dims
        self.ctx = _lib.Context.get(self.device)
        self.t = {name: torch.from_numpy(getattr(detectors, name)).to(self.device) for name in _FIELDS if name not in ("gamma", "intercept")}
        self._bound = set()

    def _bind(self, which: str):
        ctx, t = self.ctx, self.t
        if not ctx.owner_changed("emb_" + which, self) and which in self._bound:
            return
        p = _lib.ptr
        if which == "ocsvm":
            code = ctx.lib.dfa_emb_ocsvm_bind(ctx.handle, self.D, self.n_sv, p(t["mean"]), p(t["inv_scale"]), p(t["sv"]), p(t["dual_coef"]),
                                              float(self.detectors.gamma), float(self.detectors.intercept))
        else:
            code = ctx.lib.dfa_emb_gmm_bind(ctx.handle, self.D, self.P, self.K, p(t["mean"]), p(t["inv_scale"]), p(t["pca_mean"]),
                                            p(t["components"]), p(t["means"]), p(t["prec_chol"]), p(t["log_const"]))
        _lib.check(ctx.handle, code)
        self._bound.add(which)

    def _score(self, which: str, emb: torch.Tensor) -> torch.Tensor:
        if emb.device.type != "cuda":
            raise RuntimeError("dfa_amd.EmbeddingScorer scores device tensors: move the embeddings with .to('cuda')")
        if emb.dim() != 2 or emb.dtype != torch.float32:
            raise ValueError(f"embeddings must be a float32 [n, D] tensor, got {emb.dtype} {tuple(emb.shape)}")
        if emb.shape[0] == 0:
            return torch.empty(0, dtype=torch.float32, device=emb.device)
        if emb.stride(1) != 1:
            raise ValueError(f"embedding rows must be contiguous (strides {emb.stride()}); rows may be any stride >= D apart")
        N, D = emb.shape
        M, K = (self.n_sv, 0) if which == "ocsvm" else (self.P, self.K)
        with torch.cuda.device(self.ctx.index):
            self.ctx.use_current_stream()
            self._bind(which)
            ctx, lib = self.ctx, self.ctx.lib
            ws = ctx.workspace(max(256, lib.dfa_emb_workspace_bytes(_lib.EMB_OCSVM if which == "ocsvm" else _lib.EMB_GMM, N, self.D, M, K)))
            out = torch.empty(N, dtype=torch.float32, device=emb.device)
            fn = lib.dfa_emb_ocsvm_score if which == "ocsvm" else lib.dfa_emb_gmm_score
            _lib.check(ctx.handle, fn(ctx.handle, _lib.ptr(emb), N, D, emb.stride(0) if N > 1 else max(D, emb.stride(0)), _lib.ptr(out),
                                      _lib.ptr(ws), ws.numel()))
        return out

    def ocsvm_scores(self, emb: torch.Tensor) -> torch.Tensor:
        """OneClassSVM.decision_function of device embeddings [n, D] (rows any stride >= D apart) -> device float32 [n]"""
        return self._score("ocsvm", emb)

    def gmm_scores(self, emb: torch.Tensor) -> torch.Tensor:
        """GaussianMixture.score_samples(PCA.transform(.)) of device embeddings [n, D] -> device float32 [n]"""
        return self._score("gmm", emb)

    @torch.no_grad()
    def score_features(self, model: CNN2D, x: torch.Tensor, lengths=None):
        """One batch, forward and both detectors on the device: (logits [b, 1], ocsvm [b], gmm [b])."""
        kw = {} if lengths is None else {"lengths": lengths}
        logits, emb = model(x, return_embedding=True, **kw)
        return logits, self.ocsvm_scores(emb), self.gmm_scores(emb)


@torch.no_grad()
def score_file(model: CNN2D, scorer: EmbeddingScorer, features, batch_size: int = 32, device="cuda", swap_tf: bool = True,
               input_dtype=None):
    """Every utterance of a feature source (stacked tensor, or a sequence of [F, T_i] tensors: ragged where the model supports it)
    through `scorer.score_features`, batched as predict._forward_batches batches: (logits, ocsvm, gmm), each [n] on the device in
    input order; three empty tensors for an empty source."""
    from .dataloaders import EvalBatches
    source = _source(features)
    _check_ragged(model, source, swap_tf)
    model.eval()
    batches = EvalBatches(source, batch_size, device=device, dtype=input_dtype, swap_tf=swap_tf)
    outs = ([], [], [])
    for x, lengths in batches:
        logits, s_svm, s_gmm = scorer.score_features(model, x, lengths)
        for acc, v in zip(outs, (logits.squeeze(-1), s_svm, s_gmm)):
            acc.append(v)
    if not outs[0]:
        return tuple(torch.empty(0, device=device) for _ in range(3))
    return tuple(batches.restore(o) for o in outs)


def build_parser():
    p = argparse.ArgumentParser(description="Embedding-based anomaly detection using CNN2D features (MI355X HIP path).")
    p.add_argument("--checkpoint", required=True, help="Path to trained CNN2D checkpoint")
    p.add_argument("--train-features", default="data/train/features.pkl")
    p.add_argument("--train-labels", default="data/train/labels.pkl")
    p.add_argument("--dev-features", default="data/dev/features.pkl")
    p.add_argument("--dev-labels", default="data/dev/labels.pkl")
    p.add_argument("--batch-size", type=int, default=32)
    p.add_argument("--device", default=None)
    p.add_argument("--in-features", type=int, default=180)
    p.add_argument("--dropout", type=float, default=0.2)
    p.add_argument("--swap-tf", action="store_true", default=True)
    p.add_argument("--no-swap-tf", dest="swap_tf", action="store_false")
    p.add_argument("--gmm-components", type=int, default=8, help="Number of GMM components (default: 8)")
    p.add_argument("--svm-nu", type=float, default=0.05, help="OneClassSVM nu parameter (default: 0.05)")
    p.add_argument("--svm-kernel", default="rbf", help="OneClassSVM kernel (default: rbf; the only one the GPU scorer has)")
    p.add_argument("--precision", default="fp32", choices=["fp32", "bf16", "bf16x3"], help="arithmetic of the CNN2D forward")
    p.add_argument("--save-detectors", default=None, metavar="PATH", help="write the fitted detectors to this .npz")
    p.add_argument("--detectors", default=None, metavar="PATH", help="score with these fitted detectors: no fit, no sklearn")
    p.add_argument("--out", default=None, help="also write a prediction.pkl of the dev set's --score")
    p.add_argument("--score", default="ocsvm", choices=["ocsvm", "gmm"], help="which detector's score --out holds")
    return p


def parse_args(argv=None):
    args = build_parser().parse_args(argv)
    if args.svm_kernel != "rbf":
        build_parser().error(f"--svm-kernel {args.svm_kernel}: the GPU scorer implements 'rbf' alone and there is no CPU fallback")
    return args


def _labelled(features_path, labels_path):
    """(uttids, per-utterance [F, T_i] tensors, labels) of a features.pkl / labels.pkl pair, merged on uttid as
    dataset.AudioDeepfakeDataset merges them (src/dataset.py)."""
    from .dataset import AudioDeepfakeDataset
    ds = AudioDeepfakeDataset(features_path, labels_path)
    feats, labels = [], []
    for i in range(len(ds)):
        f, l = ds[i]
        feats.append(f)
        labels.append(float(l))
    return list(ds.uttids()), feats, np.asarray(labels, dtype=np.float32)


def main(argv=None):
    args = parse_args(argv)
    device = resolve_device(args.device)
    model = load_model(args.checkpoint, device, in_features=args.in_features, dropout=args.dropout, precision=args.precision)

    if args.detectors:
        detectors = Detectors.load(args.detectors)
        print(f"Loaded detectors from {args.detectors} (D, n_sv, P, K = {detectors.dims})")
    else:
        print("Extracting bonafide-only training embeddings...")
        _, train_feats, train_labels = _labelled(args.train_features, args.train_labels)
        train_emb, _ = extract_embeddings(model, train_feats, train_labels, batch_size=args.batch_size, device=device,
                                          swap_tf=args.swap_tf, bonafide_only=True)
        print(f"  Bonafide training embeddings: {train_emb.shape}")
        print(f"\nFitting One-Class SVM (nu={args.svm_nu}, kernel={args.svm_kernel})...")
        n_pca = min(256, train_emb.shape[1], train_emb.shape[0])
        print(f"Reducing to {n_pca} dims via PCA for GMM...")
        print(f"Fitting GMM (n_components={args.gmm_components})...")
        detectors = fit_detectors(train_emb, args.gmm_components, args.svm_nu, args.svm_kernel)
        if args.save_detectors:
            detectors.save(args.save_detectors)
            print(f"  Saved detectors to {args.save_detectors}")

    print("Extracting dev embeddings (both classes)...")
    uttids, dev_feats, dev_labels = _labelled(args.dev_features, args.dev_labels)
    scorer = EmbeddingScorer(detectors, device)
    _, svm_scores, gmm_scores = score_file(model, scorer, dev_feats, batch_size=args.batch_size, device=device, swap_tf=args.swap_tf)
    svm_scores, gmm_scores = svm_scores.double().cpu().numpy(), gmm_scores.double().cpu().numpy()
    print(f"  Dev embeddings: ({len(dev_feats)}, {detectors.dims[0]})")

    svm_eer, svm_thr = calculate_eer(svm_scores.tolist(), dev_labels.tolist())
    print(f"  One-Class SVM  EER = {svm_eer:.6f}  threshold = {svm_thr:.6f}")
    gmm_eer, gmm_thr = calculate_eer(gmm_scores.tolist(), dev_labels.tolist())
    print(f"  GMM            EER = {gmm_eer:.6f}  threshold = {gmm_thr:.6f}")

    print(f"\n{'=' * 60}")
    print("Embedding Anomaly Detection Results (dev set)")
    print(f"  One-Class SVM  EER = {svm_eer:.6f}")
    print(f"  GMM            EER = {gmm_eer:.6f}")
    print(f"{'=' * 60}")

    if args.out:
        from .predict import write_predictions
        write_predictions(uttids, (svm_scores if args.score == "ocsvm" else gmm_scores).tolist(), args.out)
    return {"ocsvm": svm_scores, "gmm": gmm_scores, "ocsvm_eer": svm_eer, "gmm_eer": gmm_eer}


if __name__ == "__main__":
    main()
