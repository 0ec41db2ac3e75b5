"""Refusal cases of the C ABI's training entry points (include/dfa_hip.h): the three forward_train / backward pairs, the ragged
CNN1D pair, the augmentation arming, the SyncBN hook, the losses and the optimiser.  Shared by tests/golden/make_golden_abi_errors.py
(`train` mode, which records return code and dfa_last_error text of every case) and tests/test_abi_train_errors_gpu.py (which
replays them and compares).

The rules are those of tests/abi_error_cases.py, whose Rig this one extends: every case is refused by an argument check BEFORE
any launch, in the order the entry point makes its checks; every pointer is live and large enough for the call to run in full
(neither recon nor mse, which dfa_cae_forward_train names in its own text, and neither loss nor drecon of dfa_mse_fwd_bwd are
the null-pointer cases the list needs); every case leaves the SyncBN hook cleared with fn = NULL and no augmentation armed.
A backward can only be refused for its own arguments after a forward_train of its model has run, so the rig makes a successful
forward_train (CNN2D, CNN1D uniform, CNN1D ragged, auto-encoder) at the shapes below whenever a case needs one in flight and
none is; and after every refused backward, record() runs the valid backward of the batch in flight, which must return 0: a
refusal leaves the step record as it was.  Those forwards and backwards are the list's only launches.

Shapes: B = 2; F = 20 and T = 8 for the classifiers; F = 20, T = 32 for the auto-encoder.  The training plans carry a
weight-gradient partial of about 76 MB whatever the batch: the workspace is twice the largest dfa_*_train_workspace_bytes."""
import ctypes as C

import torch

from abi_error_cases import B, F, F_WIDE, PREC_BF16, T, T_CAE, Rig, _p

F_CAE_OTHER = 36              # the auto-encoder's other legal feature dimension (16 k + 4)
NGRADS = {"cnn2d": 14, "cnn1d": 14, "cae": 30}
G_FLOATS = 1 << 19            # floats behind every gradient pointer: more than the largest parameter (256 x 128 x 9)
HOOK = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_int)


class TrainRig(Rig):
    """Rig + a training workspace, gradient buffers and a do-nothing SyncBN hook with a live 512-float buffer."""

    def __init__(self):
        super().__init__()
        lib, dev = self.lib, self.x.device
        need = [lib.dfa_cnn2d_train_workspace_bytes(self.ctx, B, T, f, PREC_BF16) for f in (F, F_WIDE)]
        need += [lib.dfa_cnn1d_train_ragged_workspace_bytes(self.ctx, B, T, f) for f in (F, F_WIDE)]
        need += [lib.dfa_cae_train_workspace_bytes(self.ctx, B, T_CAE, F, p) for p in (0, 1)]
        assert min(need) > 0
        self.tws_bytes = 2 * max(need)
        self.tws = torch.empty(self.tws_bytes, dtype=torch.uint8, device=dev)
        self.gbuf = torch.zeros(max(NGRADS.values()) * G_FLOATS, dtype=torch.float32, device=dev)
        self.grads = (C.c_void_p * max(NGRADS.values()))(*[self.gbuf.data_ptr() + 4 * G_FLOATS * i for i in range(max(NGRADS.values()))])
        self.dout = torch.zeros(1 << 16, dtype=torch.float32, device=dev)      # dlogits / drecon / loss
        self.hook_buf = torch.zeros(512, dtype=torch.float32, device=dev)
        self._hook = HOOK(lambda user, buf, count: 0)                           # world 1: the local sums are the global ones
        self.hook_armed = False
        self.inflight = dict.fromkeys(NGRADS)                                   # model -> kind of the forward_train its step record holds live
        torch.cuda.synchronize()

    # ---- state: the parent's, plus "fwd" / "fwd_ragged" = bound and that forward_train is in flight: the model's latest
    # forward_train call, successful, with no set_params and no change of the SyncBN hook since.  Whatever ends a batch in flight
    # resets `inflight` (every forward_train call, refused ones included; set_params; arming or clearing the hook) and need()
    # makes the next one.  The list keeps every forward_train case of a model before its first backward case (asserted below CASES)
    def need(self, model, state):
        if state not in ("fwd", "fwd_ragged"):
            return super().need(model, state)
        super().need(model, "params")
        if self.inflight[model] != state:
            rc = self.cnn1d_fwd(ragged=True) if state == "fwd_ragged" else getattr(self, model + "_fwd")()
            assert rc == 0, self.last_error()
            self.inflight[model] = state

    def set_params(self, model, n=None, **dims):
        if model in self.inflight:
            self.inflight[model] = None
        return super().set_params(model, n, **dims)

    def restore(self):
        """what a case may leave behind: an armed hook or augmentation"""
        assert self.arm_hook(fn=None) == 0
        for model in ("cnn2d", "cnn1d"):
            assert self.arm_augment(model, enable=0) == 0

    # ---- the calls; keyword arguments replace the good defaults ------------------------------------------------------------------------
    def _ws(self, a):
        return _p(a["ws"]), a["ws_bytes"]

    def _head(self, a):
        return self.ctx, _p(a["x"]), a["dtype"], a["B"], a["T"], a["F"], a["T"] * a["F"], a["F"], 1

    def _args(self, kw, **defaults):
        a = dict(x=self.x.data_ptr(), dtype=0, B=B, T=T, F=F, ws=self.tws.data_ptr(), ws_bytes=self.tws_bytes, p_drop=0.0,
                 lengths=[T, T], ngrads=None)
        a.update(defaults)
        a.update(kw)
        return a

    def cnn2d_fwd(self, **kw):
        self.inflight["cnn2d"] = None
        a = self._args(kw, prec=PREC_BF16)
        return self.lib.dfa_cnn2d_forward_train(*self._head(a), a["prec"], a["p_drop"], 1, 0, 0.1, 0, _p(self.out.data_ptr()), None,
                                                *self._ws(a))

    def cnn1d_fwd(self, ragged=False, **kw):
        self.inflight["cnn1d"] = None
        a = self._args(kw)
        tail = (a["p_drop"], 1, 0, 0.1, 0, _p(self.out.data_ptr()), *self._ws(a))
        if ragged:
            return self.lib.dfa_cnn1d_forward_train_ragged(*self._head(a), _p(self.lengths(a["lengths"])), *tail)
        return self.lib.dfa_cnn1d_forward_train(*self._head(a), *tail)

    def cae_fwd(self, **kw):
        self.inflight["cae"] = None
        a = self._args(kw, T=T_CAE, prec=PREC_BF16, recon=self.aux.data_ptr(), mse=self.out.data_ptr())
        return self.lib.dfa_cae_forward_train(*self._head(a), a["prec"], 0.1, 0, _p(a["recon"]), None, _p(a["mse"]), *self._ws(a))

    def bwd(self, model, ragged=False, **kw):
        a = self._args(kw, T=T_CAE if model == "cae" else T)
        n = NGRADS[model] if a["ngrads"] is None else a["ngrads"]
        fn = getattr(self.lib, f"dfa_{model}_backward" + ("_ragged" if ragged else ""))
        return fn(*self._head(a), _p(self.dout.data_ptr()), self.grads, n, *self._ws(a))

    def arm_augment(self, model, enable=1, T=T, F=F, shift=1, tm=(0, 0), fm=(0, 0), std=0.0):
        fn = getattr(self.lib, f"dfa_{model}_set_train_augment")
        return fn(self.ctx, enable, T, F, shift, None, tm[0], tm[1], fm[0], fm[1], std, 1, 0)

    def arm_hook(self, fn="hook", world=1, capacity=512):
        if fn is None:
            rc = self.lib.dfa_ctx_set_bn_sync(self.ctx, None, None, 1, None, 0)
        else:
            rc = self.lib.dfa_ctx_set_bn_sync(self.ctx, C.cast(self._hook, C.c_void_p), None, world, _p(self.hook_buf.data_ptr()), capacity)
        armed = fn is not None and rc == 0          # (a refused call leaves the hook cleared)
        if armed != self.hook_armed:
            self.inflight = dict.fromkeys(NGRADS)
        self.hook_armed = armed
        return rc

    def bce(self, smoothing=0.1, B=B):
        d = self.dout.data_ptr()
        return self.lib.dfa_bce_smooth_fwd_bwd(self.ctx, _p(self.out.data_ptr()), _p(self.aux.data_ptr()), smoothing, B, _p(d), _p(d + 256))

    def adamw(self, step=1):
        g = [_p(self.gbuf.data_ptr() + 4 * G_FLOATS * i) for i in range(4)]
        return self.lib.dfa_adamw_step(self.ctx, *g, 16, 1e-3, 0.9, 0.999, 1e-8, 0.01, step, 1.0)

    def mse(self, dtype=0, B=B, loss=True, drecon=True):
        d = self.dout.data_ptr()
        return self.lib.dfa_mse_fwd_bwd(self.ctx, _p(self.aux.data_ptr()), _p(self.x.data_ptr()), dtype, B, T_CAE, F, T_CAE * F, F, 1,
                                        _p(d) if loss else None, _p(d + 256) if drecon else None)


def _armed(r, model, call, **aug):
    assert r.arm_augment(model, **aug) == 0
    return call(r)


def _hooked(r, call):
    assert r.arm_hook() == 0
    return call(r)


def _after(r, model, what):
    """the backward of a forward_train that `what` came after: a set_params, or a forward_train refused by an argument check"""
    if what == "set_params":
        assert r.set_params(model) == 0
    else:
        assert getattr(r, model + "_fwd")(B=0) != 0
    return r.bwd(model)


def _hook_cleared(r):
    """a CNN2D forward_train under the rig's do-nothing hook (world 1), its backward with the hook cleared"""
    assert r.arm_hook() == 0
    assert r.cnn2d_fwd() == 0, r.last_error()
    assert r.arm_hook(fn=None) == 0
    return r.bwd("cnn2d")


def _cases():
    c = []

    def add(cid, model, state, fn):
        c.append((cid, model, state, fn))

    def ws_small(prefix, model, state, call):
        add(f"{prefix}/workspace_small", model, state, lambda r: call(r, ws_bytes=128))

    # ---- before anything is bound, before any forward_train has run --------------------------------------------------------------------
    add("cnn2d_forward_train/no_params", "cnn2d", "fresh", lambda r: r.cnn2d_fwd())
    add("cnn1d_forward_train/no_params", "cnn1d", "fresh", lambda r: r.cnn1d_fwd())
    add("cnn1d_forward_train_ragged/no_params", "cnn1d", "fresh", lambda r: r.cnn1d_fwd(ragged=True))
    add("cae_forward_train/no_params", "cae", "fresh", lambda r: r.cae_fwd())
    add("cnn2d_backward/no_forward", "cnn2d", "fresh", lambda r: r.bwd("cnn2d"))
    add("cnn1d_backward/no_forward", "cnn1d", "fresh", lambda r: r.bwd("cnn1d"))
    add("cnn1d_backward_ragged/no_forward", "cnn1d", "fresh", lambda r: r.bwd("cnn1d", ragged=True))
    add("cae_backward/no_forward", "cae", "fresh", lambda r: r.bwd("cae"))
    # ---- dfa_cnn2d_forward_train -----------------------------------------------------------------------------------------------------------
    add("cnn2d_forward_train/x_dtype", "cnn2d", "params", lambda r: r.cnn2d_fwd(dtype=2))
    add("cnn2d_forward_train/precision", "cnn2d", "params", lambda r: r.cnn2d_fwd(prec=3))
    add("cnn2d_forward_train/augment_other_shape", "cnn2d", "params", lambda r: _armed(r, "cnn2d", lambda r: r.cnn2d_fwd(), T=2 * T))
    add("cnn2d_forward_train/batch_0", "cnn2d", "params", lambda r: r.cnn2d_fwd(B=0))
    add("cnn2d_forward_train/T_short", "cnn2d", "params", lambda r: r.cnn2d_fwd(T=3))
    add("cnn2d_forward_train/feature_dim", "cnn2d", "params", lambda r: r.cnn2d_fwd(F=F_WIDE))
    add("cnn2d_forward_train/p_drop", "cnn2d", "params", lambda r: r.cnn2d_fwd(p_drop=1.0))
    ws_small("cnn2d_forward_train", "cnn2d", "params", lambda r, **kw: r.cnn2d_fwd(**kw))
    add("cnn2d_forward_train/workspace_misaligned", "cnn2d", "params",
        lambda r: r.cnn2d_fwd(ws=r.tws.data_ptr() + 16, ws_bytes=r.tws_bytes - 256))
    # ---- dfa_cnn1d_forward_train and _ragged -----------------------------------------------------------------------------------------------
    for ragged in (False, True):
        pre = "cnn1d_forward_train_ragged" if ragged else "cnn1d_forward_train"

        def fwd(r, ragged=ragged, **kw):
            return r.cnn1d_fwd(ragged=ragged, **kw)
        add(f"{pre}/x_dtype", "cnn1d", "params", lambda r, fwd=fwd: fwd(r, dtype=1))
        add(f"{pre}/batch_0", "cnn1d", "params", lambda r, fwd=fwd: fwd(r, B=0))
        add(f"{pre}/T_0", "cnn1d", "params", lambda r, fwd=fwd: fwd(r, T=0, lengths=[0, 0]))
        add(f"{pre}/feature_dim", "cnn1d", "params", lambda r, fwd=fwd: fwd(r, F=F_WIDE))
        add(f"{pre}/p_drop", "cnn1d", "params", lambda r, fwd=fwd: fwd(r, p_drop=1.0))
        if ragged:
            add(f"{pre}/T_short", "cnn1d", "params", lambda r, fwd=fwd: fwd(r, T=2, lengths=[2, 2]))
            add(f"{pre}/length_low", "cnn1d", "params", lambda r, fwd=fwd: fwd(r, lengths=[2, T]))
            add(f"{pre}/length_high", "cnn1d", "params", lambda r, fwd=fwd: fwd(r, lengths=[T, T + 1]))
        ws_small(pre, "cnn1d", "params", fwd)
        add(f"{pre}/augment_other_shape", "cnn1d", "params", lambda r, fwd=fwd: _armed(r, "cnn1d", fwd, T=2 * T))
        if ragged:
            add(f"{pre}/augment_armed", "cnn1d", "params", lambda r, fwd=fwd: _armed(r, "cnn1d", fwd))
            add(f"{pre}/bn_sync_armed", "cnn1d", "params", lambda r, fwd=fwd: _hooked(r, fwd))
    # ---- dfa_cae_forward_train -------------------------------------------------------------------------------------------------------------
    add("cae_forward_train/no_recon_no_mse", "cae", "params", lambda r: r.cae_fwd(recon=None, mse=None))
    add("cae_forward_train/x_dtype", "cae", "params", lambda r: r.cae_fwd(dtype=5))
    add("cae_forward_train/precision", "cae", "params", lambda r: r.cae_fwd(prec=2))
    add("cae_forward_train/batch_0", "cae", "params", lambda r: r.cae_fwd(B=0))
    add("cae_forward_train/T_short", "cae", "params", lambda r: r.cae_fwd(T=15))
    add("cae_forward_train/F_24", "cae", "params", lambda r: r.cae_fwd(F=24))
    ws_small("cae_forward_train", "cae", "params", lambda r, **kw: r.cae_fwd(**kw))
    # ---- the backwards, each after a successful forward_train of its model ----------------------------------------------------------------
    for model in ("cnn2d", "cnn1d", "cae"):
        pre, t = f"{model}_backward", (T_CAE if model == "cae" else T)
        add(f"{pre}/other_batch", model, "fwd", lambda r, m=model: r.bwd(m, B=3))
        add(f"{pre}/other_T", model, "fwd", lambda r, m=model, t=t: r.bwd(m, T=t + 2))
        if model == "cnn1d":
            add("cnn1d_backward_ragged/after_uniform_forward", model, "fwd", lambda r: r.bwd("cnn1d", ragged=True))
            add(f"{pre}/x_dtype", model, "fwd", lambda r: r.bwd("cnn1d", dtype=1))
        add(f"{pre}/gradient_count", model, "fwd", lambda r, m=model: r.bwd(m, ngrads=NGRADS[m] - 1))
        ws_small(pre, model, "fwd", lambda r, m=model, **kw: r.bwd(m, **kw))
        add(f"{pre}/other_F", model, "fwd", lambda r, m=model: r.bwd(m, F=F_CAE_OTHER if m == "cae" else F_WIDE))
        if model != "cnn1d":
            add(f"{pre}/other_x_dtype", model, "fwd", lambda r, m=model: r.bwd(m, dtype=1))
        add(f"{pre}/after_set_params", model, "fwd", lambda r, m=model: _after(r, m, "set_params"))
        add(f"{pre}/after_refused_forward", model, "fwd", lambda r, m=model: _after(r, m, "refused_forward"))
        add(f"{pre}/hook_armed_since_forward", model, "fwd", lambda r, m=model: _hooked(r, lambda r: r.bwd(m)))
    add("cnn2d_backward/hook_cleared_since_forward", "cnn2d", "fwd", _hook_cleared)
    add("cnn1d_backward/after_ragged_forward", "cnn1d", "fwd_ragged", lambda r: r.bwd("cnn1d"))
    add("cnn1d_backward_ragged/other_F", "cnn1d", "fwd_ragged", lambda r: r.bwd("cnn1d", ragged=True, F=F_WIDE))
    add("cnn1d_backward_ragged/bn_sync_armed", "cnn1d", "fwd_ragged", lambda r: _hooked(r, lambda r: r.bwd("cnn1d", ragged=True)))
    # ---- augmentation arming, SyncBN hook, losses, optimiser --------------------------------------------------------------------------------
    for model in ("cnn2d", "cnn1d"):
        pre = f"{model}_set_train_augment"
        add(f"{pre}/T_0", model, None, lambda r, m=model: r.arm_augment(m, T=0))
        add(f"{pre}/mask_outside", model, None, lambda r, m=model: r.arm_augment(m, tm=(T - 1, 2)))
        add(f"{pre}/negative_start", model, None, lambda r, m=model: r.arm_augment(m, fm=(-1, 1)))
        add(f"{pre}/jitter_negative", model, None, lambda r, m=model: r.arm_augment(m, std=-1.0))
        add(f"{pre}/jitter_nan", model, None, lambda r, m=model: r.arm_augment(m, std=float("nan")))
    add("ctx_set_bn_sync/world_0", "cnn2d", None, lambda r: r.arm_hook(world=0))
    add("ctx_set_bn_sync/capacity_511", "cnn2d", None, lambda r: r.arm_hook(capacity=511))
    add("bce_smooth_fwd_bwd/smoothing", "cnn2d", None, lambda r: r.bce(smoothing=0.5))
    add("bce_smooth_fwd_bwd/batch_0", "cnn2d", None, lambda r: r.bce(B=0))
    add("adamw_step/step_0", "cnn2d", None, lambda r: r.adamw(step=0))
    add("mse_fwd_bwd/no_loss_no_drecon", "cae", None, lambda r: r.mse(loss=False, drecon=False))
    add("mse_fwd_bwd/x_dtype", "cae", None, lambda r: r.mse(dtype=2))
    add("mse_fwd_bwd/batch_0", "cae", None, lambda r: r.mse(B=0))
    # the one refusal dfa_cnn2d_train_plan adds to the step's own (which it answers word for word: tests/test_cnn2d_train_stages_gpu.py)
    add("cnn2d_train_plan/F_0", "cnn2d", None, lambda r: r.lib.dfa_cnn2d_train_plan(r.ctx, B, T, 0, PREC_BF16, None, 0))
    # the same for dfa_cnn1d_train_plan (tests/test_cnn1d_train_stages_gpu.py)
    add("cnn1d_train_plan/F_0", "cnn1d", None, lambda r: r.lib.dfa_cnn1d_train_plan(r.ctx, B, T, 0, 0, None, 0))
    return c


CASES = _cases()
CASE_IDS = [c[0] for c in CASES]
assert len(set(CASE_IDS)) == len(CASE_IDS)
for _m in NGRADS:       # TrainRig.inflight: a model's forward_train cases all come before the first case that needs one in flight
    _first = min(i for i, c in enumerate(CASES) if c[1] == _m and c[2] in ("fwd", "fwd_ragged"))
    assert all(i < _first for i, c in enumerate(CASES) if c[1] == _m and "_forward_train" in c[0])


def record():
    """Run every case on the current device -> [[case id, return code, dfa_last_error text with pointers as PTR], ...]"""
    rig = TrainRig()
    rows = []
    try:
        for cid, model, state, fn in CASES:
            rig.need(model, state)
            rc = fn(rig)
            rows.append([cid, int(rc), rig.last_error()])
            rig.restore()
            if state in ("fwd", "fwd_ragged"):      # the refused backward left the record alone: the valid one still runs
                rig.need(model, state)
                assert rig.bwd(model, ragged=state == "fwd_ragged") == 0, (cid, rig.last_error())
    finally:
        rig.close()
    return rows
