"""Train-mode path of the HIP models (CNN2D, CNN1D, ConvAutoencoder), one bridge for all three.

Two ways to use it:
  * drop-in (reference semantics, src/train.py:71-76): `logits = model(x); loss = criterion(logits, y);
    optimizer.zero_grad(); loss.backward(); optimizer.step()` -- `model(x)` in train mode goes through `TrainFunction`, a
    torch.autograd.Function whose forward/backward are the C-ABI calls dfa_<kind>_forward_train / dfa_<kind>_backward; any
    torch criterion and optimizer work unchanged.
  * native (`NativeTrainer`, `CaeNativeTrainer`, `DlqTrainer` for the DeepfakeDetector): forward, loss, backward, ONE all-reduce of the flat gradient buffer
    (RCCL over xGMI when torch.distributed is initialised with backend "nccl") and the fused AdamW kernel,
    with no autograd graph and no per-parameter optimizer loop.
"""
from __future__ import annotations

import ctypes as C
from collections import namedtuple

import torch

from .. import _lib

KINDS = {"CNN2D": "cnn2d", "CNN1D": "cnn1d", "ConvAutoencoder": "cae"}      # model class -> C-ABI prefix / context slot

# what a raw backward needs from its forward: the context, the workspace that holds the saved activations, the forward's
# generation on the context's slot and its batch key (B, T, F, precision, x dtype, lengths of a ragged batch or None)
TrainState = namedtuple("TrainState", "ctx ws gen key")


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _train_ws(model, ctx, nbytes):
    ws = getattr(model, "_train_ws", None)
    if ws is None or ws.numel() < nbytes or ws.device.index != ctx.index:
        model._train_ws = None
        ws = torch.empty(int(nbytes), dtype=torch.uint8, device=torch.device("cuda", ctx.index))
        model._train_ws = ws
    return ws


def _bind(model, ctx, kind):
    """dfa_<kind>_set_params with the CURRENT tensors (the kernels read weights and update running stats in place)."""
    ts = model._abi_tensors()
    for t in ts:
        if t.device.type != "cuda" or t.dtype != torch.float32 or not t.is_contiguous():
            raise RuntimeError(f"{type(model).__name__} parameters must be contiguous float32 tensors on the GPU (model.to('cuda'))")
    sig = (ctx.index, tuple(t.data_ptr() for t in ts))
    if ctx.owner_changed(kind, model) or getattr(model, "_bound", None) != sig:
        dims = (model.base_channels,) if kind == "cae" else (model.in_features, model.base_channels)
        if kind == "cnn1d":     # the slot's kernel sizes are sticky: say whose model this is
            _lib.check(ctx.handle, ctx.lib.dfa_cnn1d_set_kernels(ctx.handle, *model.kernels))
        _lib.check(ctx.handle, getattr(ctx.lib, f"dfa_{kind}_set_params")(ctx.handle, _lib.ptr_array([t.detach() for t in ts]),
                                                                            len(ts), *dims))
        model._bound = sig
    model._prepared = None   # eval-mode folded images are stale after any training step


def _batch_key(model, kind, x, lengths=None):
    B, T, F = x.shape
    return (B, T, F, (None if kind == "cnn1d" else _lib.PRECISIONS[model.precision]), x.dtype,
            None if lengths is None else tuple(int(v) for v in lengths))


def _ragged_lengths(model, x, lengths):
    """Host int32 lengths of a ragged training batch, checked before anything is launched (CNN1D only in this version)."""
    if type(model).__name__ != "CNN1D":
        raise ValueError(f"variable-length (ragged) training is CNN1D only in this version, got {type(model).__name__}")
    return _lib.host_lengths(lengths, x.shape[0], x.shape[1], 3)


def _next_dropout_offset(model, n_elems):
    off = getattr(model, "_drop_offset", 0)
    model._drop_offset = off + (n_elems + 3) // 4 + 1
    return off


def forward_train_raw(model, x, want=("recon", "latent"), lengths=None):
    """One train-mode forward (dfa_<kind>_forward_train: batch statistics, running statistics updated, dropout in the
    classifiers); returns (outputs, TrainState).  outputs: (logits[B,1],) for the classifiers; for the auto-encoder the
    tensors named in `want` out of recon[B,T,F], latent[B,8C,T/16,F/16] and the per-sample mse[B], in that order.
    lengths (CNN1D): x is a ragged batch padded to T frames, utterance b is x[b, :lengths[b]] -- the step of
    dfa_cnn1d_forward_train_ragged (BatchNorm statistics over the valid frames only); `backward_raw` then runs its backward."""
    kind = KINDS[type(model).__name__]
    if lengths is not None:
        if kind == "cnn1d" and tuple(model.kernels) != (3, 3, 3):
            raise ValueError(f"CNN1D(kernels={tuple(model.kernels)}) trains on uniform batches only: the variable-length step "
                             "(lengths=...) is built for kernels=(3, 3, 3)")
        lengths = _ragged_lengths(model, x, lengths)
    if x.device.type != "cuda":
        raise RuntimeError(f"dfa_amd.{type(model).__name__} runs on the GPU only: move the input with .to('cuda')")
    if kind == "cnn1d" and x.dtype != torch.float32:
        raise ValueError(f"CNN1D takes float32 input, got {x.dtype}")
    key = _batch_key(model, kind, x, lengths)
    B, T, F, prec = key[:4]
    ctx = _lib.Context.get(x.device)
    lib, h = ctx.lib, ctx.handle
    with torch.cuda.device(ctx.index):
        ctx.use_current_stream()
        _bind(model, ctx, kind)
        ragged = "_ragged" if lengths is not None else ""
        nbytes = getattr(lib, f"dfa_{kind}_train{ragged}_workspace_bytes")(h, B, T, F, *(() if prec is None else (prec,)))
        if nbytes == 0:
            raise ValueError(f"bad {type(model).__name__} training shape (B={B}, T={T}, F={F})"
                             + (": need T >= 16 and F = 16k+4" if kind == "cae" else ""))
        ws = _train_ws(model, ctx, nbytes)
        if kind == "cae":
            shapes = {"recon": (B, T, F), "latent": (B, 8 * model.base_channels, T // 16, F // 16), "mse": (B,)}
            made = {n: torch.empty(shapes[n], dtype=torch.float32, device=x.device) for n in want}
            outs = tuple(made.values())
            args = (prec, 0.1, 1, *(_ptr(made.get(n)) for n in shapes))
            bns = [model.encoder[bi] for _, bi in model._ENC] + [model.decoder[bi] for _, bi in model._DEC if bi is not None]
        else:
            outs = (torch.empty((B, 1), dtype=torch.float32, device=x.device),)
            seed = getattr(model, "_drop_seed", None)
            if seed is None:
                seed = model._drop_seed = int(torch.initial_seed()) & 0xFFFFFFFFFFFFFFFF
            offset = _next_dropout_offset(model, B * (T // 2) * F * 32 if kind == "cnn2d" else B * 64 * T)
            args = (float(model.dropout), seed, offset, 0.1, 1, _ptr(outs[0]))
            args = (prec, *args, None) if kind == "cnn2d" else args
            bns = [model.conv[i] for i in model._BN_IDX]
        if lengths is not None:
            args = (lengths.ctypes.data_as(C.c_void_p), *args)
        _lib.check(h, getattr(lib, f"dfa_{kind}_forward_train{ragged}")(h, _ptr(x), _lib.x_dtype_code(x), B, T, F, *x.stride(), *args,
                                                                         _ptr(ws), ws.numel()))
        torch._foreach_add_([bn.num_batches_tracked for bn in bns], 1)      # one multi-tensor launch
    st = TrainState(ctx, ws, ctx.next_train_gen(kind), key)
    model.__dict__["_train_last"] = (st.gen, key)        # for the per-model entry points below (no Module.__setattr__)
    return outs, st


def backward_raw(model, x, dout, grads, st):
    """dfa_<kind>_backward of the forward that returned `st`, on that forward's batch x: WRITES (never adds) every parameter
    gradient into `grads` (one tensor per parameter, e.g. views of one flat buffer).  dout: dlogits[B,1] for the classifiers;
    for the auto-encoder drecon[B,T,F], or None when the loss is MSELoss(recon, x) (src/train_cae.py:67-68): its gradient is
    then formed inside the decoder's last backward kernel."""
    kind = KINDS[type(model).__name__]
    ctx = st.ctx
    ctx.check_train_gen(kind, st.gen, model)
    if _batch_key(model, kind, x) != (*st.key[:5], None):
        raise RuntimeError("backward called with a batch shape / precision / dtype other than its forward's")
    B, T, F = x.shape
    ragged = "_ragged" if len(st.key) > 5 and st.key[5] is not None else ""       # the forward's table is in its workspace
    with torch.cuda.device(ctx.index):
        ctx.use_current_stream()
        _lib.check(ctx.handle, getattr(ctx.lib, f"dfa_{kind}_backward{ragged}")(
            ctx.handle, _ptr(x), _lib.x_dtype_code(x), B, T, F, *x.stride(), _ptr(dout), _lib.ptr_array(grads), len(grads),
            _ptr(st.ws), st.ws.numel()))


# The per-model raw entry points other code calls (same arguments and returns as before the bridge was shared): thin
# forms of the pair above; the batch key (and CNN2D's default generation) come from the model's latest forward.
def cnn2d_forward_train_raw(model, x):
    """(logits[B,1], ctx, workspace)"""
    (logits,), st = forward_train_raw(model, x)
    return logits, st.ctx, st.ws


def cnn2d_backward_raw(model, x, dlogits, grad_tensors, ctx, ws, gen=None):
    last_gen, key = model._train_last
    backward_raw(model, x, dlogits, grad_tensors, TrainState(ctx, ws, last_gen if gen is None else gen, key))


def cae_forward_train_raw(model, x, want_recon=True, want_latent=True, want_mse=False):
    """(recon | None, latent | None, mse[B] | None, ctx, workspace, generation)"""
    names = [n for n, w in (("recon", want_recon), ("latent", want_latent), ("mse", want_mse)) if w]
    outs, st = forward_train_raw(model, x, want=names)
    got = dict(zip(names, outs))
    return got.get("recon"), got.get("latent"), got.get("mse"), st.ctx, st.ws, st.gen


def cae_backward_raw(model, x, drecon, grad_tensors, ctx, ws, gen):
    backward_raw(model, x, drecon, grad_tensors, TrainState(ctx, ws, gen, model._train_last[1]))


def _grad_dest(model):
    """(where the C backward writes each gradient, what autograd receives for it).  A parameter whose .grad is still its view
    of a FlatTrainer's flat buffer is written in place and autograd gets None: nothing is allocated, added or memset.  Any
    other parameter gets a fresh tensor that autograd accumulates as usual, so every .grad ends as plain autograd's."""
    params = list(model.parameters())
    views = model.__dict__.get("_flat_grad_sink") or [None] * len(params)
    fresh = [torch.empty_like(p) if v is None or p.grad is None or p.grad.data_ptr() != v.data_ptr() else None
             for p, v in zip(params, views)]
    return [v if g is None else g for g, v in zip(fresh, views)], fresh


class TrainFunction(torch.autograd.Function):
    """model(x) in train mode.  The auto-encoder returns (reconstruction, latent): the gradient flows through the
    reconstruction (src/train_cae.py:67-71 uses MSELoss(recon, x)), the latent map is returned for inspection only."""

    @staticmethod
    def forward(fctx, x, model, *params):
        outs, st = forward_train_raw(model, x)
        fctx.model, fctx.x, fctx.st = model, x, st
        if len(outs) == 1:
            return outs[0]
        fctx.mark_non_differentiable(*outs[1:])
        return outs

    @staticmethod
    def backward(fctx, dout, *_):
        dest, fresh = _grad_dest(fctx.model)
        backward_raw(fctx.model, fctx.x, dout.contiguous().float(), dest, fctx.st)
        return (None, None, *fresh)


def train_forward(model, x):
    return TrainFunction.apply(x, model, *model.parameters())


def cnn2d_train_forward(model, x, return_embedding=False):
    if return_embedding:
        raise NotImplementedError("return_embedding=True is an eval-mode feature (src/embedding_anomaly.py:61)")
    return train_forward(model, x)


cnn1d_train_forward = cae_train_forward = train_forward


class _FlatAdamW:
    """Parameters re-homed into ONE flat fp32 buffer (each nn.Parameter becomes a view), gradients in ONE flat buffer,
    AdamW moments alongside: the data-parallel exchange is a single all-reduce of `flat_g` and the update a single
    fused kernel (dfa_adamw_step) whatever the model (464,644 B CNN2D, 195,204 B CNN1D, 2,246,532 B auto-encoder)."""

    def __init__(self, model, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01, process_group=None):
        self.model, self.lr, self.betas, self.eps, self.wd = model, lr, betas, eps, weight_decay
        self.pg = process_group
        params = list(model.parameters())
        dev = params[0].device
        if dev.type != "cuda":
            raise RuntimeError(f"{type(self).__name__} needs the model on the GPU")
        n = sum(p.numel() for p in params)
        self.flat_p = torch.empty(n, dtype=torch.float32, device=dev)
        self.flat_g = torch.zeros(n, dtype=torch.float32, device=dev)
        self.exp_avg = torch.zeros_like(self.flat_p)
        self.exp_avg_sq = torch.zeros_like(self.flat_p)
        self.grad_views, off = [], 0
        for p in params:
            k = p.numel()
            self.flat_p[off:off + k].copy_(p.data.reshape(-1))
            p.data = self.flat_p[off:off + k].view_as(p)
            self.grad_views.append(self.flat_g[off:off + k].view_as(p))
            off += k
        self.step_count = 0
        self._sched_opt = None

    @property
    def world(self):
        import torch.distributed as dist
        return dist.get_world_size(self.pg) if (dist.is_available() and dist.is_initialized()) else 1

    def _exchange_and_update(self):
        """SUM all-reduce of the flat gradient (RCCL over xGMI under the "nccl" backend), then fused AdamW with the
        1/world scale folded in."""
        world = self.world
        if world > 1:
            import torch.distributed as dist
            dist.all_reduce(self.flat_g, op=dist.ReduceOp.SUM, group=self.pg)
        self.step_count += 1
        ctx = _lib.Context.get(self.flat_p.device)
        with torch.cuda.device(ctx.index):
            ctx.use_current_stream()
            _lib.check(ctx.handle, ctx.lib.dfa_adamw_step(
                ctx.handle, C.c_void_p(self.flat_p.data_ptr()), C.c_void_p(self.flat_g.data_ptr()),
                C.c_void_p(self.exp_avg.data_ptr()), C.c_void_p(self.exp_avg_sq.data_ptr()), self.flat_p.numel(),
                float(self.lr), float(self.betas[0]), float(self.betas[1]), float(self.eps), float(self.wd),
                self.step_count, 1.0 / world))
        self.model._prepared = None

    # ---- torch.optim.AdamW-compatible views (checkpoints stay interchangeable, src/training/checkpoint.py:42-71) ----
    def state_dict(self):
        state, off = {}, 0
        for i, p in enumerate(self.model.parameters()):
            k = p.numel()
            state[i] = {"step": torch.tensor(float(self.step_count)),
                        "exp_avg": self.exp_avg[off:off + k].view_as(p).clone(),
                        "exp_avg_sq": self.exp_avg_sq[off:off + k].view_as(p).clone()}
            off += k
        group = {"lr": self.lr, "betas": self.betas, "eps": self.eps, "weight_decay": self.wd, "amsgrad": False,
                 "maximize": False, "foreach": None, "capturable": False, "differentiable": False, "fused": None,
                 "params": list(range(len(state)))}
        return {"state": state, "param_groups": [group]}

    def load_state_dict(self, sd):
        off = 0
        for i, p in enumerate(self.model.parameters()):
            k = p.numel()
            st = sd["state"].get(i)
            if st is not None:
                self.exp_avg[off:off + k].copy_(st["exp_avg"].reshape(-1))
                self.exp_avg_sq[off:off + k].copy_(st["exp_avg_sq"].reshape(-1))
                self.step_count = int(st["step"])
            off += k
        g = sd["param_groups"][0]
        self.lr, self.betas, self.eps, self.wd = g["lr"], tuple(g["betas"]), g["eps"], g["weight_decay"]
        if self._sched_opt is not None:       # the plateau scheduler's stand-in must resume from the restored lr too
            self._sched_opt.param_groups[0]["lr"] = float(self.lr)

    def plateau_scheduler(self, **kw):
        """torch's ReduceLROnPlateau driving THIS trainer's lr (src/train.py:332-341,520-525): the scheduler owns a
        one-group stand-in optimiser whose lr is copied back after every scheduler.step(metric)."""
        trainer = self
        self._sched_opt = torch.optim.SGD([torch.zeros(1, requires_grad=True)], lr=float(self.lr))

        class _Plateau(torch.optim.lr_scheduler.ReduceLROnPlateau):
            def step(self, metrics, *a, **k):
                out = super().step(metrics, *a, **k)
                trainer.lr = float(trainer._sched_opt.param_groups[0]["lr"])
                return out
        return _Plateau(self._sched_opt, **kw)


class FlatTrainer(_FlatAdamW):
    """Optimizer-shaped data-parallel engine for any dfa_amd model used through the autograd bridge (CNN2D / CNN1D with any
    criterion, the auto-encoder with MSELoss, src/train_cae.py:58-82): `zero_grad(); loss.backward(); step()`.  Every
    parameter's .grad is a view of the flat gradient buffer, and the bridge's backward writes those gradients straight into
    the all-reduce payload (_grad_dest)."""

    def __init__(self, model, **kw):
        super().__init__(model, **kw)
        for p, g in zip(model.parameters(), self.grad_views):
            p.grad = g
        model.__dict__["_flat_grad_sink"] = self.grad_views

    def zero_grad(self, set_to_none: bool = False):
        """Re-attach the views; no memset: the dfa_*_backward calls WRITE every gradient whose .grad is its view, and a
        detached one gets a fresh tensor (one backward per step on this path)."""
        for p, g in zip(self.model.parameters(), self.grad_views):
            if p.grad is None or p.grad.data_ptr() != g.data_ptr():
                p.grad = g

    def step(self):
        self._exchange_and_update()


class NativeTrainer(_FlatAdamW):
    """Whole classifier training step on the C ABI: forward_train -> BCE(smoothed) -> backward (gradients written straight
    into the views of the flat buffer) -> all-reduce -> fused AdamW, with no autograd graph (src/train.py:71-76).
    CNN2D and CNN1D (chosen by the model's class).
    sync_bn (world > 1): BatchNorm statistics over the GLOBAL batch (two 2C-float all-reduces per layer and step through the
    C ABI's hook, armed for this trainer's forward / backward only): N ranks x B then train like one rank x N*B; the default
    is DistributedDataParallel's local statistics."""

    def __init__(self, model, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01, label_smoothing=0.0,
                 process_group=None, sync_bn=False):
        if not (0.0 <= label_smoothing < 0.5):
            raise ValueError("--label-smoothing must be in [0, 0.5)")          # src/train.py:308-309
        super().__init__(model, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, process_group=process_group)
        self.label_smoothing = label_smoothing
        self.bn_sync = _lib.BnSync(self.flat_p.device, process_group) if sync_bn and self.world > 1 else None
        self.loss_buf = torch.zeros(1, dtype=torch.float32, device=self.flat_p.device)
        self.dlogits = None
        self.kind = KINDS[type(model).__name__]

    def step(self, x, y, lengths=None):
        """One optimisation step on batch (x[B,T,F], y[B]); returns the (device) loss scalar of this rank's batch.
        lengths (CNN1D, one rank): x is a ragged batch padded to T frames, utterance b is x[b, :lengths[b]]; the step is the
        reference model's on the utterances concatenated along time (BatchNorm statistics over the valid frames, the time mean
        over each utterance's own frames); frames past an utterance's length are never used."""
        model = self.model
        if lengths is not None:                 # refused before anything is launched: the model class, SyncBN, the lengths
            lengths = _ragged_lengths(model, x, lengths)
            if self.bn_sync is not None:
                raise ValueError("variable-length (ragged) training does not support sync_bn on more than one rank: the ranks' "
                                 "frame counts differ and the synchronisation hook carries sums only")
        model.train()
        if self.bn_sync is not None:
            self.bn_sync.arm()
        try:
            (logits,), st = forward_train_raw(model, x, lengths=lengths)
            B = x.shape[0]
            if self.dlogits is None or self.dlogits.numel() != B:
                self.dlogits = torch.empty(B, dtype=torch.float32, device=x.device)
            y = y.to(device=x.device, dtype=torch.float32).contiguous()
            ctx = st.ctx
            with torch.cuda.device(ctx.index):
                _lib.check(ctx.handle, ctx.lib.dfa_bce_smooth_fwd_bwd(
                    ctx.handle, _ptr(logits), _ptr(y), float(self.label_smoothing), B, _ptr(self.loss_buf), _ptr(self.dlogits)))
            backward_raw(model, x, self.dlogits, self.grad_views, st)
        finally:
            if self.bn_sync is not None:
                self.bn_sync.disarm()
        self._exchange_and_update()
        return self.loss_buf


class CaeNativeTrainer(_FlatAdamW):
    """Whole auto-encoder training step on the C ABI (src/train_cae.py:58-82: recon = model(x); MSELoss(recon, x); backward;
    AdamW): forward_train writes only the per-sample MSE, the backward forms 2 (recon - x) / N inside its first kernel
    (dfa_cae_backward with drecon = NULL) and writes the 30 gradients straight into the flat buffer, then ONE 2,246,532-byte
    all-reduce and the fused AdamW.  No reconstruction, no loss gradient, no autograd graph and no torch elementwise kernel.
    sync_bn: as NativeTrainer's."""

    def __init__(self, model, lr=1e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-4, process_group=None, sync_bn=False):
        super().__init__(model, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, process_group=process_group)
        self.bn_sync = _lib.BnSync(self.flat_p.device, process_group) if sync_bn and self.world > 1 else None

    def step(self, x):
        """One optimisation step on the (z-scored) batch x[B,T,F]; returns the device scalar MSELoss(recon, x) of this rank."""
        model = self.model
        model.train()
        if self.bn_sync is not None:
            self.bn_sync.arm()
        try:
            (mse,), st = forward_train_raw(model, x, want=("mse",))
            backward_raw(model, x, None, self.grad_views, st)
        finally:
            if self.bn_sync is not None:
                self.bn_sync.disarm()
        self._exchange_and_update()
        return mse.mean()          # every sample has T*F elements: the mean of the per-sample MSEs is nn.MSELoss's mean


class DlqTrainer(_FlatAdamW):
    """Whole DeepfakeDetector training step on the C ABI (src/dlqueen_model.py:255-330 without AMP: everything is fp32-grade,
    GradScaler / autocast have no counterpart): dfa_dlq_forward_train -> BCEWithLogitsLoss(pos_weight) -> dfa_dlq_backward into the
    flat gradient views -> clip_grad_norm_(grad_clip) on the device -> fused AdamW -> EMA of the parameters.  The step is dense
    over the padded batch as the reference's is: BatchNorm1d counts every frame of x[B, C, T_max], padding included, so a step
    depends on the batch's composition and on T_max.  One rank only in this version."""

    def __init__(self, model, lr=1e-3, weight_decay=1e-4, pos_weight=1.0, grad_clip=5.0, ema_decay=None):
        if type(model).__name__ != "DeepfakeDetector":
            raise ValueError(f"DlqTrainer trains a dfa_amd DeepfakeDetector, got {type(model).__name__}")
        super().__init__(model, lr=lr, weight_decay=weight_decay)
        if self.world > 1:
            raise ValueError("DlqTrainer runs on one rank in this version: the DeepfakeDetector step has no gradient exchange and no "
                             "synchronised BatchNorm yet")
        self.pos_weight, self.grad_clip, self.ema_decay = float(pos_weight), float(grad_clip), ema_decay
        dev = self.flat_p.device
        self.loss_buf = torch.zeros(1, dtype=torch.float32, device=dev)
        self.norm_buf = torch.zeros(1, dtype=torch.float32, device=dev)
        self.dlogits = None
        self.shadow = self.flat_p.clone() if ema_decay is not None else None
        self.keep_out = None        # test hook: a uint8 tensor of 3 * B * 256 * T + B * 256 elements receives the keep bits

    def step(self, x, lengths, y):
        """One optimisation step on (x[B, C, T_max] float32 in the stored layout, lengths[B], y[B] in {0, 1}); returns the device
        loss scalar.  Frames of x behind an utterance's end are taken as zero and never used."""
        model = self.model
        if x.dim() != 3:
            raise ValueError(f"DeepfakeDetector expects x of shape (B, C, T), got {tuple(x.shape)}")
        _lib.require_gpu(model, x)
        B, Cc, T = x.shape
        lengths = _lib.host_lengths(lengths, B, T, 1)
        x = _lib.stored_layout(x, model._conforms(x), time_last=True)
        sb, sc, _ = x.stride()
        model.train()
        ctx = _lib.Context.get(x.device)
        lib, h = ctx.lib, ctx.handle
        with torch.cuda.device(ctx.index):
            ctx.use_current_stream()
            ts = model._abi_tensors()
            sig = (ctx.index, tuple(t.data_ptr() for t in ts))
            if ctx.owner_changed("dlq", model) or getattr(model, "_bound", None) != sig:
                _lib.check(h, lib.dfa_dlq_set_params(h, _lib.ptr_array([t.detach() for t in ts]), len(ts), model.in_ch, model.hidden))
                model._bound = sig
            model._prepared = None          # the eval images are stale after this step
            nbytes = lib.dfa_dlq_train_workspace_bytes(h, B, T, Cc)
            if nbytes == 0:
                raise ValueError(f"bad DeepfakeDetector training shape (B={B}, C={Cc}, T_max={T}): BatchNorm1d needs B * T_max >= 2")
            ws = _train_ws(model, ctx, nbytes)
            if self.dlogits is None or self.dlogits.numel() != B:
                self.dlogits = torch.empty(B, dtype=torch.float32, device=x.device)
                self.logits = torch.empty(B, dtype=torch.float32, device=x.device)
            seed = getattr(model, "_drop_seed", None)
            if seed is None:
                seed = model._drop_seed = int(torch.initial_seed()) & 0xFFFFFFFFFFFFFFFF
            offset = _next_dropout_offset(model, B * 256 * T)
            y = y.to(device=x.device, dtype=torch.float32).contiguous()
            lp = C.c_void_p(lengths.ctypes.data)
            _lib.check(h, lib.dfa_dlq_forward_train(h, _ptr(x), B, T, Cc, sb, sc, lp, float(model.dropout), seed, offset, 0.1, 1,
                                                    _ptr(self.logits), _ptr(self.keep_out), _ptr(ws), ws.numel()))
            torch._foreach_add_([model.enc.net[i].num_batches_tracked for i in model._BN_IDX], 1)
            _lib.check(h, lib.dfa_bce_pos_weight_fwd_bwd(h, _ptr(self.logits), _ptr(y), self.pos_weight, B, _ptr(self.loss_buf),
                                                         _ptr(self.dlogits)))
            _lib.check(h, lib.dfa_dlq_backward(h, _ptr(x), B, T, Cc, sb, sc, _ptr(self.dlogits), _lib.ptr_array(self.grad_views),
                                               len(self.grad_views), _ptr(ws), ws.numel()))
            if self.grad_clip > 0:
                _lib.check(h, lib.dfa_clip_grad_norm(h, _ptr(self.flat_g), self.flat_g.numel(), self.grad_clip, _ptr(self.norm_buf)))
        self._exchange_and_update()
        if self.shadow is not None:
            self.shadow.lerp_(self.flat_p, 1.0 - self.ema_decay)
        return self.loss_buf

    def ema_applied(self):
        """Context manager: the EMA shadow in place of the weights (for evaluation), the weights restored on exit."""
        import contextlib

        @contextlib.contextmanager
        def swap():
            if self.shadow is None:
                yield
                return
            saved = self.flat_p.clone()
            self.flat_p.copy_(self.shadow)
            self.model._prepared = None
            try:
                yield
            finally:
                self.flat_p.copy_(saved)
                self.model._prepared = None
        return swap()


def make_cae_trainer(model, **kw):
    return CaeNativeTrainer(model, **kw)
