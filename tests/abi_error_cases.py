"""Refusal cases of the C ABI's eval entry points (include/dfa_hip.h), shared by tests/golden/make_golden_abi_errors.py (which
records return code and dfa_last_error text of every case) and tests/test_abi_errors_gpu.py (which replays them and compares).

Every case is refused by an argument check BEFORE any launch, in the order the entry point makes its checks.  Two rules keep a
check that went missing a failed comparison instead of a fault: every pointer a case passes -- x, workspace, outputs, statistics
and the weight tensors, which are those of models as wide as the widest feature dimension any case names -- points into live
memory large enough for the call to run in full ("misaligned" = a 4- or 16-byte offset into a larger allocation, "too small" =
a smaller byte count for the full buffer), and no case passes a null data pointer, null lengths or a capturing stream (mu without sigma, which the
auto-encoder entry points name in their own message, is the one exception the list needs).

Shapes are the smallest the checks accept: B = 2; in_features / in_ch = 20 and T = 8 for CNN2D, CNN1D and DeepfakeDetector;
F = 20 (16 * 1 + 4) and T = 32 for the auto-encoder."""
import ctypes as C
import re

import numpy as np
import torch

B, F, T, T_CAE = 2, 20, 8, 32
F_WIDE = 24             # the widest feature dimension a case passes
PREC_F32, PREC_BF16 = 0, 1
# the options the ragged entry points insist on, with their defaults (dfa_internal.h: struct dfa_ctx)
OPTION_DEFAULTS = {"fuse_conv1": 1, "block3_m16": 1, "cnn1d_fused": 1, "cae_dec_fused": 1, "cae_enc1_mfma": 1, "cae_enc_dma": 1,
                   "lds_pipe": 1}
X_FLOATS = 1 << 20          # every x the cases describe, wrong ones included, lies inside this many floats
WS_BYTES = 16 << 20


def _p(v):
    return C.c_void_p(int(v)) if v is not None else None


class Rig:
    """One dfa_ctx of its own, the four models' parameter tensors and buffers far larger than any case needs."""

    def __init__(self):
        from dfa_amd import _lib
        from dfa_amd.dlqueen_model import DeepfakeDetector
        from dfa_amd.model import CNN2D
        from dfa_amd.model_cae import ConvAutoencoder
        from dfa_amd.model_cnn1d import CNN1D
        self.lib = lib = _lib.load()
        dev = torch.device("cuda", torch.cuda.current_device())
        self.ctx = C.c_void_p()
        assert lib.dfa_ctx_create(dev.index, None, C.byref(self.ctx)) == 0
        # (the weights are those of models F_WIDE features wide, bound as F: a feature-dim case whose check went missing stays inside them)
        models = {"cnn2d": CNN2D(in_features=F_WIDE), "cnn1d": CNN1D(in_features=F_WIDE), "cae": ConvAutoencoder(),
                  "dlq": DeepfakeDetector(F_WIDE)}
        self.tensors = {k: [t.detach() for t in m.to(dev)._abi_tensors()] for k, m in models.items()}
        self.arrays = {k: _lib.ptr_array(ts) for k, ts in self.tensors.items()}
        self.x = torch.zeros(X_FLOATS, dtype=torch.float32, device=dev)
        self.ws = torch.empty(WS_BYTES, dtype=torch.uint8, device=dev)
        self.out = torch.zeros(1 << 16, dtype=torch.float32, device=dev)       # logits / mse
        self.aux = torch.zeros(1 << 16, dtype=torch.float32, device=dev)       # embedding / pooled
        self.mu = torch.zeros(64, dtype=torch.float32, device=dev)
        self.sigma = torch.ones(64, dtype=torch.float32, device=dev)
        self.state = dict.fromkeys(models, "fresh")
        self._lengths = None
        for model, (t, prec) in {"cnn2d": (T, PREC_BF16), "cnn1d": (T, PREC_F32), "cae": (T_CAE, PREC_BF16)}.items():
            code = {"cnn2d": 0, "cnn1d": 1, "cae": 2}[model]
            assert 2 * lib.dfa_workspace_bytes(self.ctx, code, B, t, F + 4, prec) <= WS_BYTES
        assert 2 * lib.dfa_dlq_workspace_bytes(self.ctx, B, T, F) <= WS_BYTES
        torch.cuda.synchronize()

    def close(self):
        torch.cuda.synchronize()
        assert self.lib.dfa_ctx_destroy(self.ctx) == 0

    # ---- model state: "fresh" (nothing bound; only before the first bind), "params" (bound, not prepared), PREC_* / "ready" -------
    def set_params(self, model, n=None, **dims):
        lib, arr = self.lib, self.arrays[model]
        n = len(self.tensors[model]) if n is None else n
        if model == "cae":
            return lib.dfa_cae_set_params(self.ctx, arr, n, dims.get("base_channels", 32))
        if model == "dlq":
            return lib.dfa_dlq_set_params(self.ctx, arr, n, dims.get("in_ch", F), dims.get("hidden", 256))
        fn = lib.dfa_cnn2d_set_params if model == "cnn2d" else lib.dfa_cnn1d_set_params
        return fn(self.ctx, arr, n, dims.get("in_features", F), dims.get("base_channels", 32))

    def prepare(self, model, prec=None):
        lib = self.lib
        if model == "cnn2d":
            return lib.dfa_cnn2d_prepare(self.ctx, prec)
        if model == "cae":
            return lib.dfa_cae_prepare(self.ctx, prec)
        return (lib.dfa_cnn1d_prepare if model == "cnn1d" else lib.dfa_dlq_prepare)(self.ctx)

    def need(self, model, state):
        if state is None or self.state[model] == state:
            return
        assert state != "fresh", f"{model}: a 'fresh' case after the model was bound"
        assert self.set_params(model) == 0
        if state != "params":
            assert self.prepare(model, None if state == "ready" else state) == 0
        self.state[model] = state

    def rebind(self, model, **dims):
        """bind and prepare with other dimensions (the same, large enough, tensors); the next need() restores the usual ones"""
        assert self.set_params(model, **dims) == 0 and self.prepare(model) == 0
        self.state[model] = "other"

    def set_option(self, name, value):
        return self.lib.dfa_ctx_set_option(self.ctx, name.encode(), value)

    def last_error(self):
        return re.sub(r"0x[0-9a-fA-F]+", "PTR", self.lib.dfa_last_error(self.ctx).decode())

    def lengths(self, values):
        self._lengths = np.ascontiguousarray(values, dtype=np.int32)      # (kept alive until the next call)
        return self._lengths.ctypes.data

    # ---- the seven forwards; keyword arguments replace the good defaults ----------------------------------------------------------
    def cnn2d(self, ragged=False, **kw):
        a = dict(x=self.x.data_ptr(), dtype=0, B=B, T=T, F=F, sb=T * F, st=F, sf=1, lengths=[T, T], emb=None, ws=self.ws.data_ptr(),
                 ws_bytes=WS_BYTES)
        a.update(kw)
        head = (self.ctx, _p(a["x"]), a["dtype"], a["B"], a["T"], a["F"], a["sb"], a["st"], a["sf"])
        tail = (_p(self.out.data_ptr()), _p(a["emb"]), _p(a["ws"]), a["ws_bytes"])
        if ragged:
            return self.lib.dfa_cnn2d_forward_ragged(*head, _p(self.lengths(a["lengths"])), *tail)
        return self.lib.dfa_cnn2d_forward(*head, *tail)

    def cnn1d(self, ragged=False, **kw):
        # ragged: the stored channel-major batch [B][F][T] seen as [B, T, F]
        a = dict(x=self.x.data_ptr(), dtype=0, B=B, T=T, F=F, lengths=[T, T], ws=self.ws.data_ptr(), ws_bytes=WS_BYTES,
                 **(dict(sb=F * T, st=1, sf=T) if ragged else dict(sb=T * F, st=F, sf=1)))
        a.update(kw)
        head = (self.ctx, _p(a["x"]), a["dtype"], a["B"], a["T"], a["F"], a["sb"], a["st"], a["sf"])
        tail = (_p(self.out.data_ptr()), _p(a["ws"]), a["ws_bytes"])
        if ragged:
            return self.lib.dfa_cnn1d_forward_ragged(*head, _p(self.lengths(a["lengths"])), *tail)
        return self.lib.dfa_cnn1d_forward(*head, *tail)

    def cae(self, ragged=False, **kw):
        a = dict(x=self.x.data_ptr(), dtype=0, B=B, T=T_CAE, F=F, st=None, sf=1, lengths=[T_CAE, T_CAE], mu=self.mu.data_ptr(),
                 sigma=self.sigma.data_ptr(), ws=self.ws.data_ptr(), ws_bytes=WS_BYTES)
        a.update(kw)
        st = a["F"] if a["st"] is None else a["st"]
        head = (self.ctx, _p(a["x"]), a["dtype"], a["B"], a["T"], a["F"], a["T"] * a["F"], st, a["sf"])
        stats = (_p(a["mu"]), _p(a["sigma"]))
        tail = (_p(self.out.data_ptr()), _p(a["ws"]), a["ws_bytes"])
        if ragged:
            return self.lib.dfa_cae_score_ragged(*head, _p(self.lengths(a["lengths"])), *stats, *tail)
        return self.lib.dfa_cae_forward(*head, *stats, None, None, *tail)

    def dlq(self, **kw):
        a = dict(x=self.x.data_ptr(), B=B, T=T, C=F, sb=F * T, sc=T, lengths=[T, T], ws=self.ws.data_ptr(), ws_bytes=WS_BYTES)
        a.update(kw)
        return self.lib.dfa_dlq_forward(self.ctx, _p(a["x"]), a["B"], a["T"], a["C"], a["sb"], a["sc"], _p(self.lengths(a["lengths"])),
                                        _p(self.out.data_ptr()), _p(self.aux.data_ptr()), _p(a["ws"]), a["ws_bytes"])


def _cnn1d_f18(r):
    r.rebind("cnn1d", in_features=18)
    return r.cnn1d(ragged=True, F=18, sb=18 * T)


def _mid(r):
    return r.x.data_ptr() + 2 * X_FLOATS     # the middle of x: a negative stride stays inside it


def _common_ws(call, prefix, model, state):
    """workspace too small / misaligned, for a forward that checks both"""
    return [
        (f"{prefix}/workspace_small", model, state, {}, lambda r: call(r, ws_bytes=128)),
        (f"{prefix}/workspace_misaligned", model, state, {}, lambda r: call(r, ws=r.ws.data_ptr() + 16, ws_bytes=WS_BYTES - 256)),
    ]


def _cases():
    c = []

    def add(cid, model, state, fn, **opts):
        c.append((cid, model, state, opts, fn))

    # ---- before anything is bound ---------------------------------------------------------------------------------------------------
    add("cnn2d_prepare/no_params", "cnn2d", "fresh", lambda r: r.prepare("cnn2d", PREC_BF16))
    add("cnn1d_prepare/no_params", "cnn1d", "fresh", lambda r: r.prepare("cnn1d"))
    add("cae_prepare/no_params", "cae", "fresh", lambda r: r.prepare("cae", PREC_BF16))
    add("dlq_prepare/no_params", "dlq", "fresh", lambda r: r.prepare("dlq"))
    # ---- set_params, in the order of its checks ---------------------------------------------------------------------------------------
    add("cnn2d_set_params/count", "cnn2d", None, lambda r: r.set_params("cnn2d", n=19))
    add("cnn2d_set_params/base_channels", "cnn2d", None, lambda r: r.set_params("cnn2d", base_channels=64))
    add("cnn2d_set_params/in_features", "cnn2d", None, lambda r: r.set_params("cnn2d", in_features=0))
    add("cnn1d_set_params/count", "cnn1d", None, lambda r: r.set_params("cnn1d", n=21))
    add("cnn1d_set_params/base_channels", "cnn1d", None, lambda r: r.set_params("cnn1d", base_channels=16))
    add("cnn1d_set_params/in_features", "cnn1d", None, lambda r: r.set_params("cnn1d", in_features=-3))
    add("cae_set_params/count", "cae", None, lambda r: r.set_params("cae", n=43))
    add("cae_set_params/base_channels", "cae", None, lambda r: r.set_params("cae", base_channels=48))
    add("dlq_set_params/count", "dlq", None, lambda r: r.set_params("dlq", n=20))
    add("dlq_set_params/hidden", "dlq", None, lambda r: r.set_params("dlq", hidden=128))
    add("dlq_set_params/in_ch_mod4", "dlq", None, lambda r: r.set_params("dlq", in_ch=18))
    add("dlq_set_params/in_ch_small", "dlq", None, lambda r: r.set_params("dlq", in_ch=0))
    add("dlq_set_params/in_ch_large", "dlq", None, lambda r: r.set_params("dlq", in_ch=260))
    # ---- bound, not prepared ----------------------------------------------------------------------------------------------------------
    add("cnn2d_prepare/precision", "cnn2d", "params", lambda r: r.prepare("cnn2d", 3))
    add("cae_prepare/precision", "cae", "params", lambda r: r.prepare("cae", 2))
    add("cnn2d_forward/not_prepared", "cnn2d", "params", lambda r: r.cnn2d())
    add("cnn2d_forward_ragged/not_prepared", "cnn2d", "params", lambda r: r.cnn2d(ragged=True))
    add("cnn1d_forward/not_prepared", "cnn1d", "params", lambda r: r.cnn1d())
    add("cnn1d_forward_ragged/not_prepared", "cnn1d", "params", lambda r: r.cnn1d(ragged=True))
    add("cae_forward/not_prepared", "cae", "params", lambda r: r.cae())
    add("cae_score_ragged/not_prepared", "cae", "params", lambda r: r.cae(ragged=True))
    add("dlq_forward/not_prepared", "dlq", "params", lambda r: r.dlq())
    # ---- dfa_cnn2d_forward --------------------------------------------------------------------------------------------------------------
    add("cnn2d_forward/x_dtype", "cnn2d", PREC_BF16, lambda r: r.cnn2d(dtype=2))
    add("cnn2d_forward/batch_0", "cnn2d", PREC_BF16, lambda r: r.cnn2d(B=0))
    add("cnn2d_forward/feature_dim", "cnn2d", PREC_BF16, lambda r: r.cnn2d(F=24, st=24, sb=T * 24))
    add("cnn2d_forward/T_short", "cnn2d", PREC_BF16, lambda r: r.cnn2d(T=3))
    c.extend(_common_ws(lambda r, **kw: r.cnn2d(**kw), "cnn2d_forward", "cnn2d", PREC_BF16))
    add("cnn2d_forward/embedding_misaligned", "cnn2d", PREC_BF16, lambda r: r.cnn2d(emb=r.aux.data_ptr() + 4))
    add("cnn2d_forward/workspace_small_f32", "cnn2d", PREC_F32, lambda r: r.cnn2d(ws_bytes=512))
    # ---- dfa_cnn2d_forward_ragged -------------------------------------------------------------------------------------------------------
    add("cnn2d_forward_ragged/x_dtype", "cnn2d", PREC_BF16, lambda r: r.cnn2d(ragged=True, dtype=-1))
    add("cnn2d_forward_ragged/batch_0", "cnn2d", PREC_BF16, lambda r: r.cnn2d(ragged=True, B=0))
    add("cnn2d_forward_ragged/feature_dim", "cnn2d", PREC_BF16, lambda r: r.cnn2d(ragged=True, F=16, st=16, sb=T * 16))
    add("cnn2d_forward_ragged/T_short", "cnn2d", PREC_BF16, lambda r: r.cnn2d(ragged=True, T=3, lengths=[3, 3]))
    add("cnn2d_forward_ragged/length_low", "cnn2d", PREC_BF16, lambda r: r.cnn2d(ragged=True, lengths=[T, 3]))
    add("cnn2d_forward_ragged/length_high", "cnn2d", PREC_BF16, lambda r: r.cnn2d(ragged=True, lengths=[T + 1, T]))
    add("cnn2d_forward_ragged/precision_f32", "cnn2d", PREC_F32, lambda r: r.cnn2d(ragged=True))
    add("cnn2d_forward_ragged/fuse_conv1_0", "cnn2d", PREC_BF16, lambda r: r.cnn2d(ragged=True), fuse_conv1=0)
    add("cnn2d_forward_ragged/block3_m16_0", "cnn2d", PREC_BF16, lambda r: r.cnn2d(ragged=True), block3_m16=0)
    c.extend(_common_ws(lambda r, **kw: r.cnn2d(ragged=True, **kw), "cnn2d_forward_ragged", "cnn2d", PREC_BF16))
    add("cnn2d_forward_ragged/embedding_misaligned", "cnn2d", PREC_BF16, lambda r: r.cnn2d(ragged=True, emb=r.aux.data_ptr() + 8))
    # ---- dfa_cnn1d_forward (checks the workspace's size only) -----------------------------------------------------------------------------
    add("cnn1d_forward/x_dtype", "cnn1d", "ready", lambda r: r.cnn1d(dtype=1))
    add("cnn1d_forward/batch_0", "cnn1d", "ready", lambda r: r.cnn1d(B=0))
    add("cnn1d_forward/T_0", "cnn1d", "ready", lambda r: r.cnn1d(T=0))
    add("cnn1d_forward/feature_dim", "cnn1d", "ready", lambda r: r.cnn1d(F=24, st=24, sb=T * 24))
    add("cnn1d_forward/workspace_small", "cnn1d", "ready", lambda r: r.cnn1d(ws_bytes=256))
    # ---- dfa_cnn1d_forward_ragged -------------------------------------------------------------------------------------------------------
    add("cnn1d_forward_ragged/x_dtype", "cnn1d", "ready", lambda r: r.cnn1d(ragged=True, dtype=1))
    add("cnn1d_forward_ragged/batch_0", "cnn1d", "ready", lambda r: r.cnn1d(ragged=True, B=0))
    add("cnn1d_forward_ragged/feature_dim", "cnn1d", "ready", lambda r: r.cnn1d(ragged=True, F=24, sb=24 * T))
    add("cnn1d_forward_ragged/T_short", "cnn1d", "ready", lambda r: r.cnn1d(ragged=True, T=2, lengths=[2, 2]))
    add("cnn1d_forward_ragged/length_low", "cnn1d", "ready", lambda r: r.cnn1d(ragged=True, lengths=[2, T]))
    add("cnn1d_forward_ragged/length_high", "cnn1d", "ready", lambda r: r.cnn1d(ragged=True, lengths=[T, T + 1]))
    add("cnn1d_forward_ragged/stride_t", "cnn1d", "ready", lambda r: r.cnn1d(ragged=True, sb=T * F, st=F, sf=1))
    add("cnn1d_forward_ragged/F_mod4", "cnn1d", None, _cnn1d_f18)
    add("cnn1d_forward_ragged/stride_f_mod4", "cnn1d", "ready", lambda r: r.cnn1d(ragged=True, sf=T + 2, sb=F * (T + 2)))
    add("cnn1d_forward_ragged/stride_f_short", "cnn1d", "ready", lambda r: r.cnn1d(ragged=True, sf=4))
    add("cnn1d_forward_ragged/stride_b_mod4", "cnn1d", "ready", lambda r: r.cnn1d(ragged=True, sb=F * T + 2))
    add("cnn1d_forward_ragged/stride_b_negative", "cnn1d", "ready", lambda r: r.cnn1d(ragged=True, x=_mid(r), sb=-F * T))
    add("cnn1d_forward_ragged/x_misaligned", "cnn1d", "ready", lambda r: r.cnn1d(ragged=True, x=r.x.data_ptr() + 4))
    add("cnn1d_forward_ragged/cnn1d_fused_0", "cnn1d", "ready", lambda r: r.cnn1d(ragged=True), cnn1d_fused=0)
    add("cnn1d_forward_ragged/cnn1d_fused_2", "cnn1d", "ready", lambda r: r.cnn1d(ragged=True), cnn1d_fused=2)
    c.extend(_common_ws(lambda r, **kw: r.cnn1d(ragged=True, **kw), "cnn1d_forward_ragged", "cnn1d", "ready"))
    # ---- dfa_cae_forward ----------------------------------------------------------------------------------------------------------------
    add("cae_forward/mu_without_sigma", "cae", PREC_BF16, lambda r: r.cae(sigma=None))
    add("cae_forward/x_dtype", "cae", PREC_BF16, lambda r: r.cae(dtype=5))
    add("cae_forward/batch_0", "cae", PREC_BF16, lambda r: r.cae(B=0))
    add("cae_forward/T_short", "cae", PREC_BF16, lambda r: r.cae(T=15))
    add("cae_forward/F_24", "cae", PREC_BF16, lambda r: r.cae(F=24))
    c.extend(_common_ws(lambda r, **kw: r.cae(**kw), "cae_forward", "cae", PREC_BF16))
    add("cae_forward/workspace_small_f32", "cae", PREC_F32, lambda r: r.cae(ws_bytes=1024))
    # ---- dfa_cae_score_ragged -----------------------------------------------------------------------------------------------------------
    add("cae_score_ragged/sigma_without_mu", "cae", PREC_BF16, lambda r: r.cae(ragged=True, mu=None))
    add("cae_score_ragged/x_dtype", "cae", PREC_BF16, lambda r: r.cae(ragged=True, dtype=2))
    add("cae_score_ragged/batch_0", "cae", PREC_BF16, lambda r: r.cae(ragged=True, B=0))
    add("cae_score_ragged/T_short", "cae", PREC_BF16, lambda r: r.cae(ragged=True, T=15, lengths=[15, 15]))
    add("cae_score_ragged/length_low", "cae", PREC_BF16, lambda r: r.cae(ragged=True, lengths=[T_CAE, 15]))
    add("cae_score_ragged/length_high", "cae", PREC_BF16, lambda r: r.cae(ragged=True, lengths=[T_CAE + 1, 16]))
    add("cae_score_ragged/precision_f32", "cae", PREC_F32, lambda r: r.cae(ragged=True))
    add("cae_score_ragged/F_24", "cae", PREC_BF16, lambda r: r.cae(ragged=True, F=24))
    for name in ("cae_dec_fused", "cae_enc1_mfma", "cae_enc_dma", "lds_pipe"):
        add(f"cae_score_ragged/{name}_0", "cae", PREC_BF16, lambda r: r.cae(ragged=True), **{name: 0})
    add("cae_score_ragged/stride_negative", "cae", PREC_BF16, lambda r: r.cae(ragged=True, x=_mid(r), st=-F))
    c.extend(_common_ws(lambda r, **kw: r.cae(ragged=True, **kw), "cae_score_ragged", "cae", PREC_BF16))
    # ---- dfa_dlq_forward ----------------------------------------------------------------------------------------------------------------
    add("dlq_forward/batch_0", "dlq", "ready", lambda r: r.dlq(B=0))
    add("dlq_forward/T_0", "dlq", "ready", lambda r: r.dlq(T=0, lengths=[0, 0]))
    add("dlq_forward/channel_dim", "dlq", "ready", lambda r: r.dlq(C=24))
    add("dlq_forward/length_low", "dlq", "ready", lambda r: r.dlq(lengths=[T, 0]))
    add("dlq_forward/length_high", "dlq", "ready", lambda r: r.dlq(lengths=[T + 1, T]))
    add("dlq_forward/stride_c_mod4", "dlq", "ready", lambda r: r.dlq(sc=T + 2, sb=F * (T + 2)))
    add("dlq_forward/stride_c_short", "dlq", "ready", lambda r: r.dlq(sc=4))
    add("dlq_forward/stride_b_mod4", "dlq", "ready", lambda r: r.dlq(sb=F * T + 1))
    add("dlq_forward/stride_b_negative", "dlq", "ready", lambda r: r.dlq(x=_mid(r), sb=-F * T))
    add("dlq_forward/x_misaligned", "dlq", "ready", lambda r: r.dlq(x=r.x.data_ptr() + 8))
    c.extend(_common_ws(lambda r, **kw: r.dlq(**kw), "dlq_forward", "dlq", "ready"))
    # ---- options ------------------------------------------------------------------------------------------------------------------------
    add("ctx_set_option/unknown", "cnn2d", None, lambda r: r.set_option("no_such_option", 1))
    add("ctx_set_option/unknown_empty", "cnn2d", None, lambda r: r.set_option("", 0))
    return c


CASES = _cases()
CASE_IDS = [c[0] for c in CASES]
assert len(set(CASE_IDS)) == len(CASE_IDS)


def record():
    """Run every case on the current device -> [[case id, return code, dfa_last_error text with pointers as PTR], ...]"""
    rig = Rig()
    rows = []
    try:
        for cid, model, state, opts, fn in CASES:
            rig.need(model, state)
            for name, value in opts.items():
                assert rig.set_option(name, value) == 0, name
            try:
                rc = fn(rig)
            finally:
                for name in opts:
                    assert rig.set_option(name, OPTION_DEFAULTS[name]) == 0, name
            rows.append([cid, int(rc), rig.last_error()])
    finally:
        rig.close()
    return rows
