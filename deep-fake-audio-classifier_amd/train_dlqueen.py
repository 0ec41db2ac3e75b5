"""Training CLI of the DeepfakeDetector on the MI355X -- counterpart of the training half of the reference's
src/dlqueen_model.py:255-411, on the all-C-ABI step (training.DlqTrainer: dfa_dlq_forward_train, BCEWithLogitsLoss(pos_weight),
dfa_dlq_backward, gradient clip, fused AdamW, EMA).

Same arguments and data layout (data/<split>/features.pkl + labels.pkl).  What is kept of the reference's loop: class weights and
pos_weight = neg / pos, a WeightedRandomSampler with replacement, batches in SAMPLER ORDER padded to the batch's longest utterance
(the step depends on the batch's composition, so there is no length sorting), per-sample SpecAugment on the host before staging,
dev EER every epoch (file-order batches, under the EMA weights with --ema), the best state_dict saved with torch.save under the
reference's keys and shapes (the raw weights, as the reference saves them after restoring from the EMA), early stopping.
What is not: AMP.  The step is fp32-grade throughout; GradScaler / autocast have no counterpart.

--resident (default off): both splits are uploaded once (dataloaders.DlqResidentSet) and every batch is assembled on the device by
one launch; the host still draws the sampler's order and the SpecAugment masks (draw_spans), so the run is bit for bit the same
(DESIGN.md section 3.15b)."""
from __future__ import annotations

import argparse
import os
import random

import numpy as np
import torch


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description="DeepfakeDetector (Conv1d + StatsPool) training on the MI355X")
    ap.add_argument("--data_dir", default="data")
    ap.add_argument("--train_split", default="train")
    ap.add_argument("--dev_split", default="dev")
    ap.add_argument("--ckpt_path", default="best_model.pth")
    ap.add_argument("--device", default="cuda")
    ap.add_argument("--seed", type=int, default=42)
    ap.add_argument("--epochs", type=int, default=30)
    ap.add_argument("--batch_size", type=int, default=32)
    ap.add_argument("--lr", type=float, default=1e-3)
    ap.add_argument("--weight_decay", type=float, default=1e-4)
    ap.add_argument("--grad_clip", type=float, default=5.0)
    ap.add_argument("--hidden", type=int, default=256)
    ap.add_argument("--dropout", type=float, default=0.3)
    ap.add_argument("--specaug", action="store_true", help="enable SpecAugment during training")
    ap.add_argument("--time_mask_max", type=int, default=30)
    ap.add_argument("--time_mask_n", type=int, default=2)
    ap.add_argument("--freq_mask_max", type=int, default=24)
    ap.add_argument("--freq_mask_n", type=int, default=2)
    ap.add_argument("--ema", action="store_true")
    ap.add_argument("--ema_decay", type=float, default=0.999)
    ap.add_argument("--patience", type=int, default=6)
    ap.add_argument("--resident", action="store_true",
                    help="keep the train and dev sets in GPU memory and assemble every batch there (dataloaders.DlqResidentSet)")
    from .normalization import add_norm_argument
    add_norm_argument(ap)
    args = ap.parse_args(argv)
    if args.hidden != 256:
        ap.exit(2, f"--hidden {args.hidden}: the DeepfakeDetector HIP path is built for hidden=256\n")
    if args.epochs < 1:
        ap.exit(2, "--epochs must be >= 1 (prediction from a checkpoint: python -m dfa_amd.dlqueen_model)\n")
    if args.batch_size < 1:
        ap.exit(2, "--batch_size must be >= 1\n")
    if not 0.0 <= args.dropout < 1.0:
        ap.exit(2, "--dropout must be in [0, 1)\n")
    if args.resident and args.specaug and sum(span_counts(args.time_mask_max, args.time_mask_n, args.freq_mask_max, args.freq_mask_n)) > 16:
        ap.exit(2, "--resident: the batch gather takes at most 16 mask spans per utterance (time_mask_n + freq_mask_n <= 16)\n")
    return args


def compute_class_weights(labels):
    """(pos_weight = neg / pos, weight of a class-0 sample, of a class-1 sample): src/dlqueen_model.py:255-264"""
    labels = np.asarray(labels)
    pos, neg = int((labels == 1).sum()), int((labels == 0).sum())
    return float(neg / max(pos, 1)), 1.0 / max(neg, 1), 1.0 / max(pos, 1)


def sample_order(labels, generator):
    """one epoch's sample indices: WeightedRandomSampler(class weights, len(labels), replacement=True)"""
    _, w0, w1 = compute_class_weights(labels)
    w = torch.tensor([w1 if int(v) == 1 else w0 for v in labels], dtype=torch.double)
    return torch.multinomial(w, len(labels), replacement=True, generator=generator).tolist()


def spec_augment(x, rng, time_mask_max, time_mask_n, freq_mask_max, freq_mask_n):
    """the reference's time_mask then freq_mask on one [C, T] sample, in place (src/dlqueen_model.py:33-62); rng: random.Random"""
    Cc, T = x.shape
    if time_mask_max > 0:
        for _ in range(max(time_mask_n, 0)):
            w = rng.randint(0, min(time_mask_max, T))
            if w == 0:
                continue
            t0 = rng.randint(0, max(0, T - w))
            x[:, t0:t0 + w] = 0.0
    if freq_mask_max > 0:
        for _ in range(max(freq_mask_n, 0)):
            w = rng.randint(0, min(freq_mask_max, Cc))
            if w == 0:
                continue
            c0 = rng.randint(0, max(0, Cc - w))
            x[c0:c0 + w, :] = 0.0
    return x


def epoch_batches(feats, labels, order, batch_size, specaug=None, rng=None, norm: str = "raw", device=None):
    """Batches of one epoch in the order given (no sorting): (x [b, C, T] host float32 in the stored layout, zero behind every
    utterance, rows padded to 16 bytes; lengths int32 [b]; y float32 [b]).  specaug: (time_mask_max, time_mask_n, freq_mask_max,
    freq_mask_n) applied per sample to a copy, or None.
    norm "cmn" / "cvmn" (needs `device`): x is then a DEVICE tensor -- the unmasked batch is uploaded, every utterance normalised
    there over its own frames, and the masks, drawn as spans by the same rng in the same order (draw_spans), zero the normalised
    data: the reference's order (its dataset normalises, its loop masks), and what a DlqResidentSet(norm=...) batch holds."""
    if norm != "raw" and device is None:
        raise ValueError("epoch_batches(norm=...) normalises on the GPU: pass device=")
    for lo in range(0, len(order), batch_size):
        idx = order[lo:lo + batch_size]
        utts = [torch.as_tensor(feats[i]).float() for i in idx]
        lengths = np.array([u.shape[-1] for u in utts], dtype=np.int32)
        T = int(lengths.max())
        host = torch.zeros((len(utts), utts[0].shape[0], -(-T // 4) * 4), dtype=torch.float32)
        if norm != "raw":
            from .normalization import normalize_batch
            n_t = span_counts(*specaug)[0] if specaug is not None else 0
            spans = [draw_spans(rng, u.shape[0], u.shape[-1], *specaug) for u in utts] if specaug is not None else None
            for j, u in enumerate(utts):
                host[j, :, :u.shape[-1]] = u
            xt = host.to(device).transpose(1, 2)                   # [b, T_pad, C]: the stored batch, read and written in place
            x = normalize_batch(xt, norm, lengths, out=xt).transpose(1, 2)
            for j, sp in enumerate(spans or ()):
                for k, (s0, w) in enumerate(sp.tolist()):
                    if w and k < n_t:
                        x[j, :, s0:s0 + w] = 0.0
                    elif w:
                        x[j, s0:s0 + w, :] = 0.0
            yield x[:, :, :T], lengths, torch.tensor([float(labels[i]) for i in idx], dtype=torch.float32)
            continue
        for j, u in enumerate(utts):
            if specaug is not None:
                u = spec_augment(u.clone(), rng, *specaug)
            host[j, :, :u.shape[-1]] = u
        yield host[:, :, :T], lengths, torch.tensor([float(labels[i]) for i in idx], dtype=torch.float32)


def span_counts(time_mask_max, time_mask_n, freq_mask_max, freq_mask_n):
    """(time spans, channel spans) draw_spans records per sample: a family with max <= 0 or n <= 0 has none"""
    return (time_mask_n if time_mask_max > 0 and time_mask_n > 0 else 0), (freq_mask_n if freq_mask_max > 0 and freq_mask_n > 0 else 0)


def draw_spans(rng, C, T, time_mask_max, time_mask_n, freq_mask_max, freq_mask_n):
    """spec_augment's masks of one [C, T] sample as spans instead of slice assignments: int32 [n_t + n_f, 2] = (start, width),
    the time spans first (span_counts).  Consumes rng in exactly spec_augment's order -- per mask w = randint(0, min(max, dim)),
    the start only when w != 0 -- so one rng drives either; a mask of width 0 is recorded as (0, 0)."""
    n_t, n_f = span_counts(time_mask_max, time_mask_n, freq_mask_max, freq_mask_n)
    out = np.zeros((n_t + n_f, 2), dtype=np.int32)
    for k in range(n_t + n_f):
        cap, dim = (time_mask_max, T) if k < n_t else (freq_mask_max, C)
        w = rng.randint(0, min(cap, dim))
        if w == 0:
            continue
        out[k] = (rng.randint(0, max(0, dim - w)), w)
    return out


def resident_epoch_batches(rset, order, batch_size, specaug=None, rng=None):
    """epoch_batches on a dataloaders.DlqResidentSet: the same triples in the same order, bit for bit, assembled on the device
    (x [b, C, T] device float32 in the stored layout, lengths int32 [b] on the host, y float32 [b] on the device).  The spans
    are drawn sample by sample in batch order, as epoch_batches draws its masks: one rng drives both paths identically.  x is
    the set's one batch buffer: consume a batch before asking for the next."""
    n_t = span_counts(*specaug)[0] if specaug is not None else 0
    for lo in range(0, len(order), batch_size):
        idx = order[lo:lo + batch_size]
        spans = None
        if specaug is not None:
            spans = np.stack([draw_spans(rng, rset.C, int(rset.lengths[i]), *specaug) for i in idx])
        yield rset.batch(idx, spans, n_t)


def train_epoch(trainer, batches, device):
    """mean of the steps' losses (one host read at the end of the epoch)"""
    losses = []
    for x, lengths, y in batches:
        losses.append(trainer.step(x.to(device), lengths, y).clone())
    return float(torch.stack(losses).mean().item()) if losses else float("nan")


def _load_split(data_dir, split):
    import pandas as pd
    df = pd.read_pickle(os.path.join(data_dir, split, "features.pkl"))
    lab = pd.read_pickle(os.path.join(data_dir, split, "labels.pkl"))
    if "uttid" not in df.columns or "features" not in df.columns:
        raise ValueError(f"{split}/features.pkl needs the columns 'uttid' and 'features'")
    label_map = dict(zip(lab["uttid"].tolist(), lab["label"].tolist()))
    feats = [torch.as_tensor(f) for f in df["features"].tolist()]
    return feats, np.array([int(label_map[u]) for u in df["uttid"].tolist()], dtype=int)


def dlq_checkpoint(model, norm: str = "raw"):
    """What train_dlqueen saves: the bare state_dict the reference's script saves and loads; with "cmn" / "cvmn" (which the
    reference's script cannot reproduce) {"model_state": state_dict, "norm_mode": mode}, which dfa_amd.dlqueen_model resolves."""
    state = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
    return state if norm == "raw" else {"model_state": state, "norm_mode": norm}


def main(argv=None):
    from .dataloaders import DlqResidentSet
    from .dlqueen_model import DeepfakeDetector, evaluate_eer, evaluate_eer_resident
    from .training import DlqTrainer

    args = parse_args(argv)
    random.seed(args.seed)
    np.random.seed(args.seed)
    torch.manual_seed(args.seed)
    train_feats, y_train = _load_split(args.data_dir, args.train_split)
    dev_feats, y_dev = _load_split(args.data_dir, args.dev_split)
    pos_weight, _, _ = compute_class_weights(y_train)
    if args.resident and not DlqResidentSet.fits(list(train_feats) + list(dev_feats), args.device):
        raise SystemExit(f"--resident: the packed train and dev sets do not fit in half of the free memory of '{args.device}'; "
                         "run without --resident")
    model = DeepfakeDetector(in_ch=int(train_feats[0].shape[0]), hidden=args.hidden, dropout=args.dropout).to(args.device)
    model._drop_seed, model._drop_offset = int(args.seed) & 0xFFFFFFFFFFFFFFFF, 0
    trainer = DlqTrainer(model, lr=args.lr, weight_decay=args.weight_decay, pos_weight=pos_weight, grad_clip=args.grad_clip,
                         ema_decay=args.ema_decay if args.ema else None)
    gen = torch.Generator().manual_seed(args.seed)
    rng = random.Random(args.seed)
    specaug = (args.time_mask_max, args.time_mask_n, args.freq_mask_max, args.freq_mask_n) if args.specaug else None
    best_eer, bad = 1.0, 0
    if args.resident:           # both splits uploaded once; from here on the host sends indices and mask spans only
        train_set = DlqResidentSet(train_feats, y_train, device=args.device, norm=args.norm)
        dev_set = DlqResidentSet(dev_feats, None, device=args.device, norm=args.norm)
    for epoch in range(1, args.epochs + 1):
        order = sample_order(y_train, gen)
        if args.resident:
            loss = train_epoch(trainer, resident_epoch_batches(train_set, order, args.batch_size, specaug, rng), args.device)
        else:
            loss = train_epoch(trainer, epoch_batches(train_feats, y_train, order, args.batch_size, specaug, rng, norm=args.norm,
                                                      device=args.device), args.device)
        with trainer.ema_applied():
            if args.resident:
                dev_eer = evaluate_eer_resident(model, dev_set, y_dev, args.batch_size)
            else:
                dev_eer = evaluate_eer(model, dev_feats, y_dev, args.batch_size, device=args.device, file_order=True, norm=args.norm)
        print(f"Epoch {epoch}: train_loss={loss:.6f} dev EER={dev_eer:.6f}  (lower is better)")
        if dev_eer < best_eer:
            best_eer, bad = dev_eer, 0
            torch.save(dlq_checkpoint(model, args.norm), args.ckpt_path)
            print(f"  Saved best ckpt -> {args.ckpt_path}")
        else:
            bad += 1
            if bad >= args.patience:
                print(f"Early stopping: no improvement for {args.patience} epochs.")
                break
    print(f"\nTraining done. Best dev EER: {best_eer:.6f}")


if __name__ == "__main__":
    main()
