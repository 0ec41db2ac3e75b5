"""Checkpoint -> prediction.pkl -- counterpart of src/predict.py (same CLI flags, same output schema: DataFrame
{uttid, predictions} with Python-float scores, sigmoid applied by default), with the forward on the MI355X HIP path.

    python -m dfa_amd.predict --features features.pkl --checkpoint cnn2d_best.pt --model cnn2d --out prediction.pkl
"""
from __future__ import annotations

import argparse

import pandas as pd
import torch

from .model import CNN2D


def build_model(name: str, in_features: int = 180, dropout: float = 0.3, precision: str = "fp32", kernels=(3, 3, 3)):
    if name == "cnn2d":
        return CNN2D(in_features=in_features, dropout=dropout, precision=precision)
    if name == "cnn1d":
        from .model_cnn1d import CNN1D
        return CNN1D(in_features=in_features, dropout=dropout, kernels=kernels)
    raise ValueError(f"unknown model {name!r} (choices: cnn2d, cnn1d)")


def read_checkpoint(checkpoint_path: str, device="cuda"):
    """What torch.load finds in the file: the reference's checkpoint dict or a bare state_dict."""
    try:
        return torch.load(checkpoint_path, map_location=device, weights_only=True)
    except TypeError:
        return torch.load(checkpoint_path, map_location=device)


def load_weights(model, checkpoint_path: str, device="cuda", blob=None):
    """Accept the reference's checkpoint dict {"model_state": ...} or a bare state_dict (src/predict.py:78-85).
    blob: the file's content when the caller has read it already (read_checkpoint)."""
    ckpt = read_checkpoint(checkpoint_path, device) if blob is None else blob
    state = ckpt["model_state"] if isinstance(ckpt, dict) and "model_state" in ckpt else ckpt
    model.load_state_dict(state)
    return model


def _forward_batches(model, source, batch_size, device, rank, world, input_dtype, swap_tf=True, return_embedding=False,
                     norm: str = "raw"):
    """The one scoring loop: `source` (a stacked tensor or a list of [F, T_i] tensors: dataloaders.EvalBatches) through
    `model(x)` / `model(x, lengths=...)` -> (logits [n] on the device, embeddings [n, 128*F] on the host or None), in input
    order; (None, None) when this rank's shard is empty.  norm: "cmn" / "cvmn" normalise each batch where it reaches the
    device, every utterance over the stored time axis and its own frames (float32 input)."""
    from .dataloaders import EvalBatches
    from .normalization import normalize_batch, normalize_stored
    model.eval()
    batches = EvalBatches(source, batch_size, device=device, rank=rank, world=world, dtype=input_dtype, swap_tf=swap_tf)
    outs, embs = [], []
    for x, lengths in batches:
        kw = {} if lengths is None else {"lengths": lengths}
        if norm != "raw":
            if lengths is not None:
                x = normalize_batch(x, norm, lengths, out=x)           # the padded batch's own device copy: in place
            else:
                x = normalize_batch(x, norm) if swap_tf else normalize_stored(x, norm)
        if return_embedding:
            logits, e = model(x, return_embedding=True, **kw)
            embs.append(e.cpu())
        else:
            logits = model(x, **kw)
        outs.append(logits.squeeze(-1))
    if not outs:
        return None, None
    return batches.restore(outs), (batches.restore(embs) if embs else None)


@torch.no_grad()
def predict_scores(model, features: torch.Tensor, batch_size: int = 32, device="cuda", apply_sigmoid: bool = True,
                   swap_tf: bool = True, rank: int = 0, world: int = 1, input_dtype=None, norm: str = "raw") -> torch.Tensor:
    """Scores for a stacked [N,180,321] feature tensor (this rank's shard when world > 1), as one GPU tensor."""
    logits, _ = _forward_batches(model, features, batch_size, device, rank, world, input_dtype, swap_tf, norm=norm)
    if logits is None:
        return torch.empty(0, device=device)
    return torch.sigmoid(logits) if apply_sigmoid else logits


def check_ragged_args(model: str, precision: str, swap_tf: bool = True) -> None:
    """Can a features.pkl whose utterances differ in length be scored with these arguments?  Raises ValueError when not:
    cnn1d scores ragged files as it is; cnn2d has ragged kernels for --precision bf16 only; and the stored [F, T_i] layout
    is the only ragged layout, so --no-swap-tf is refused.  Pure: touches neither the GPU nor the file."""
    if not swap_tf:
        raise ValueError("features.pkl holds utterances of unequal lengths: --no-swap-tf is not supported for such a file "
                         "(the stored [F, T] layout is the only ragged layout)")
    if model == "cnn2d" and precision != "bf16":
        raise ValueError(f"features.pkl holds utterances of unequal lengths: --model cnn2d scores such a file with "
                         f"--precision bf16 only (got --precision {precision}); --model cnn1d takes any length")
    if model not in ("cnn2d", "cnn1d"):
        raise ValueError(f"unknown model {model!r} (choices: cnn2d, cnn1d)")


@torch.no_grad()
def predict_scores_ragged(model, feature_list, batch_size: int = 32, device="cuda", apply_sigmoid: bool = True,
                          input_dtype=None, rank: int = 0, world: int = 1, return_embedding: bool = False, norm: str = "raw"):
    """Scores for a list of per-utterance [F, T_i] tensors of unequal lengths, in input order, as one GPU tensor: batches
    padded to their longest utterance (dataloaders.RaggedBatcher, longest first) through `model(x, lengths=...)`.
    return_embedding (cnn2d): also the [N, 128*F] embeddings, as a host tensor.  norm: see _forward_batches."""
    logits, emb = _forward_batches(model, feature_list, batch_size, device, rank, world, input_dtype,
                                   return_embedding=return_embedding, norm=norm)
    if logits is None:
        scores = torch.empty(0, device=device)
    else:
        scores = torch.sigmoid(logits) if apply_sigmoid else logits
    if return_embedding:
        return scores, (emb if emb is not None else torch.empty(0, 0))
    return scores


@torch.no_grad()
def extract_embeddings(model, features: torch.Tensor, batch_size: int = 256, device="cuda", swap_tf: bool = True,
                       rank: int = 0, world: int = 1, input_dtype=None, norm: str = "raw"):
    """Bulk export of the block-3 time-mean embedding [N, 128*F] (what src/embedding_anomaly.py:49-73 collects with
    forward hooks for its OC-SVM / GMM stage) together with the logits [N]: the HIP forward writes the embedding rows
    straight from the block-3 epilogue (`return_embedding=True`), so the export costs one extra 92 KB store per utterance.
    Returns (embeddings, logits) as host tensors (this rank's shard when world > 1)."""
    if not isinstance(model, CNN2D):
        raise ValueError("extract_embeddings needs the CNN2D model (the 1D CNN has no [128*F] embedding)")
    logits, emb = _forward_batches(model, features, batch_size, device, rank, world, input_dtype, swap_tf, return_embedding=True,
                                   norm=norm)
    if logits is None:
        return torch.empty(0, 0), torch.empty(0)
    return emb, logits.cpu()


def write_predictions(uttids, scores, out_path: str) -> pd.DataFrame:
    """prediction.pkl exactly as src/predict.py:116-122 writes it (uttid object column, float64 predictions)."""
    scores = [float(s) for s in scores]
    if len(scores) != len(uttids):
        raise ValueError("Number of predictions does not match number of rows in features.pkl")
    df = pd.DataFrame({"uttid": uttids, "predictions": scores})
    df.to_pickle(out_path)
    return df


def build_submission(features_df: pd.DataFrame, prediction_df: pd.DataFrame, student_id: str, first_name: str,
                     last_name: str, nickname: str) -> dict:
    """The submission dict of scripts/generate_submission.py:17-48, with the same checks and error messages:
    {student_id, first_name, last_name, nickname, predictions: DataFrame{uttid, predictions float64}}."""
    import numpy as np
    if len(prediction_df.columns) != 2:
        raise ValueError("prediction.pkl must have exactly 2 columns")
    if "uttid" not in prediction_df.columns or "predictions" not in prediction_df.columns:
        raise ValueError("prediction.pkl must have 'uttid' and 'predictions' columns")
    if "uttid" not in features_df.columns:
        raise ValueError("features.pkl must have 'uttid' column")
    if set(features_df["uttid"].values) != set(prediction_df["uttid"].values):
        raise ValueError("uttid mismatch between features.pkl and prediction.pkl")
    if not all(isinstance(x, (float, np.floating)) for x in prediction_df["predictions"].values):
        prediction_df = prediction_df.copy()
        prediction_df["predictions"] = prediction_df["predictions"].astype(np.float64)
    return {"student_id": student_id, "first_name": first_name, "last_name": last_name, "nickname": nickname,
            "predictions": prediction_df}


def write_submission(features_path: str, prediction_path: str, student_id: str, first_name: str, last_name: str,
                     nickname: str, out_dir: str = ".") -> str:
    """Counterpart of `python scripts/generate_submission.py features.pkl prediction.pkl ID First Last Nick`
    (:38-53): pickles the dict as <ID>-<First>-<Last>-<Nick>.pkl and returns the path."""
    import os
    import pickle
    result = build_submission(pd.read_pickle(features_path), pd.read_pickle(prediction_path), student_id, first_name,
                              last_name, nickname)
    path = os.path.join(out_dir, f"{student_id}-{first_name}-{last_name}-{nickname}.pkl")
    with open(path, "wb") as fh:
        pickle.dump(result, fh)
    return path


def parse_args(argv=None):
    p = argparse.ArgumentParser(description="Generate prediction.pkl from a model checkpoint (MI355X HIP path).")
    p.add_argument("--features", required=True, help="Path to features.pkl")
    p.add_argument("--checkpoint", required=True, help="Path to model checkpoint")
    p.add_argument("--model", required=True, choices=["cnn2d", "cnn1d"])
    p.add_argument("--out", required=True, help="Output path for prediction.pkl")
    p.add_argument("--batch-size", type=int, default=32)
    p.add_argument("--num-workers", type=int, default=2)
    p.add_argument("--device", default=None, help="cuda (the HIP path has no CPU fallback)")
    _add_embedding_flag(p)
    p.add_argument("--in-features", type=int, default=180)
    p.add_argument("--dropout", type=float, default=0.3)
    p.add_argument("--apply-sigmoid", action="store_true", default=True)
    p.add_argument("--no-apply-sigmoid", action="store_true", default=False)
    p.add_argument("--precision", default="fp32", choices=["fp32", "bf16", "bf16x3"])
    from .normalization import add_norm_argument
    add_norm_argument(p)          # not given: the checkpoint's "norm_mode", else raw (normalization.resolve_norm)
    p.add_argument("--kernels", default=None, metavar="K1,K2,K3",
                   help="--model cnn1d: Conv1d kernel sizes, 3,3,3 or 5,3,3 (src/compare_kernels.py's CNN1D_Variant); "
                        "not given: the checkpoint's \"kernels\", else 3,3,3")
    sw = p.add_mutually_exclusive_group()
    sw.add_argument("--swap-tf", dest="swap_tf", action="store_true", help="swap time and feature dims (default)")
    sw.add_argument("--no-swap-tf", dest="swap_tf", action="store_false")
    p.set_defaults(swap_tf=True)
    return p.parse_args(argv)


def _add_embedding_flag(p):
    p.add_argument("--embeddings-out", default=None,
                   help="also write the block-3 embeddings [N, 128*F] (+ uttids, logits) to this .pt file (cnn2d only)")


def check_kernels_arg(model: str, kernels_text):
    """--kernels as a tuple (None when not given).  Pure -- called before a model or a file is touched: ValueError for a model
    other than cnn1d or a set the HIP path is not built for."""
    if kernels_text is None:
        return None
    if model != "cnn1d":
        raise ValueError(f"--kernels is a --model cnn1d flag (got --model {model}): only the 1D CNN has the k = (5, 3, 3) variant")
    from .model_cnn1d import parse_kernels
    return parse_kernels(kernels_text)


def main(argv=None):
    from . import distributed as _dist
    _dist.limit_cpu_threads()      # the job's CPU share, not the machine's CPU count (distributed.cpu_budget)
    args = parse_args(argv)
    kernels_flag = check_kernels_arg(args.model, args.kernels)
    device = args.device or "cuda"
    apply_sigmoid = False if args.no_apply_sigmoid else args.apply_sigmoid
    features_df = pd.read_pickle(args.features)
    if "uttid" not in features_df.columns:
        raise ValueError("features.pkl must contain 'uttid'")
    ragged = len({tuple(f.shape) for f in features_df["features"]}) > 1      # utterances of unequal lengths
    if ragged:
        check_ragged_args(args.model, args.precision, args.swap_tf)
    from .normalization import explicit_norm, resolve_norm
    if args.model == "cnn1d":          # its kernel sizes may come from the checkpoint: the file is read first
        from .model_cnn1d import resolve_kernels
        blob = read_checkpoint(args.checkpoint, device)
        model = build_model(args.model, args.in_features, args.dropout, args.precision,
                            kernels=resolve_kernels(kernels_flag, blob)).to(device)
    else:                              # as before: a model the arguments do not allow is refused before the file is read
        model = build_model(args.model, args.in_features, args.dropout, args.precision).to(device)
        blob = read_checkpoint(args.checkpoint, device)
    load_weights(model, args.checkpoint, device, blob=blob)
    norm = resolve_norm(explicit_norm(args), blob)
    model.eval()
    if ragged:
        feature_list = [f.float() for f in features_df["features"]]
        scores = predict_scores_ragged(model, feature_list, batch_size=args.batch_size, device=device,
                                       apply_sigmoid=apply_sigmoid, norm=norm)
        write_predictions(features_df["uttid"].values, scores.cpu().tolist(), args.out)
        if args.embeddings_out:
            if args.model != "cnn2d":
                raise ValueError("extract_embeddings needs the CNN2D model (the 1D CNN has no [128*F] embedding)")
            logits, emb = predict_scores_ragged(model, feature_list, batch_size=max(args.batch_size, 256), device=device,
                                                apply_sigmoid=False, return_embedding=True, norm=norm)
            torch.save({"uttid": list(features_df["uttid"].values), "embeddings": emb, "logits": logits.cpu()},
                       args.embeddings_out)
        return
    feats = torch.stack([f.float() for f in features_df["features"]]) if len(features_df) else torch.empty(0, 180, 321)
    scores = predict_scores(model, feats, batch_size=args.batch_size, device=device, apply_sigmoid=apply_sigmoid,
                            swap_tf=args.swap_tf, norm=norm)
    write_predictions(features_df["uttid"].values, scores.cpu().tolist(), args.out)
    if args.embeddings_out:
        emb, logits = extract_embeddings(model, feats, batch_size=max(args.batch_size, 256), device=device, swap_tf=args.swap_tf,
                                         norm=norm)
        torch.save({"uttid": list(features_df["uttid"].values), "embeddings": emb, "logits": logits}, args.embeddings_out)


if __name__ == "__main__":
    main()
