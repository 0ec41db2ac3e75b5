"""Exact-size workspaces between canary bands -- TEST INFRASTRUCTURE ONLY (a plain helper module, imported by
tests/test_workspace_bounds_gpu.py).

Every entry point of the C ABI writes its intermediates into a caller-supplied workspace whose size the ABI's planners state
(dfa_workspace_bytes and its siblings).  The library's own Python keeps grow-only workspaces (Context.workspace, _train_ws), so
after one large call every later small one runs with megabytes of slack and an overrun of the stated size lands in it unseen.
Here a call gets EXACTLY the planner's byte count, cut out of the middle of one larger allocation:

    [ band: pad bytes of 0x5A ][ interior: nbytes of 0xFF ][ band: pad bytes of 0x5A ]

pad = max(1 MiB, nbytes) rounded up to 256: a band at least as large as the whole workspace keeps an overrun of any ONE region of
the plan inside the allocation, so a wrong kernel fails an assertion instead of faulting the card.  The interior's 0xFF bytes are
NaN both as bf16 (0xFFFF) and as fp32 (0xFFFFFFFF): a kernel that reads a workspace slot nobody wrote gives a result that differs
from a run on a workspace of finite bytes.

`eval_workspace` / `train_workspace` inject the interior view without touching the library's Python: Context.workspace(n) returns
ctx._ws unchanged whenever ctx._ws.numel() >= n, and _train_ws(model, ctx, n) does the same with model._train_ws; both callers
pass ws.numel() to the ABI, which is therefore told exactly nbytes.  Both managers assert on exit that the library still holds
the injected view: had the planner asked for more than nbytes, the library would have replaced it silently and the bands would
guard nothing."""
import contextlib

import torch

MIB = 1 << 20
FINITE = 0x3C            # 0x3C3C = 0.0115 as bf16, 0x3C3C3C3C = 0.0115 as fp32: the "earlier finite bytes" of a roomy workspace


def _damage(region, band):
    """(first, last) index of a byte of `region` that no longer holds `band`, or None"""
    bad = region != band
    if not bool(bad.any()):
        return None
    idx = bad.nonzero()
    return int(idx[0]), int(idx[-1])


def banded(nbytes, interior=0xFF, band=0x5A, device="cuda"):
    """-> (view, check): `view` is a uint8 tensor of exactly `nbytes` bytes filled with `interior`, 256-byte aligned, with
    max(1 MiB, nbytes) bytes of `band` in front of it and behind it in the same allocation.  check(what="") synchronises and
    asserts that both bands still hold `band`; a failure names the first and last damaged byte as offsets from the END of the
    workspace (0 = the first byte behind it; anything below -nbytes lies in front of it)."""
    nbytes = int(nbytes)
    pad = -(-max(MIB, nbytes) // 256) * 256
    buf = torch.empty(pad + nbytes + pad, dtype=torch.uint8, device=device)
    assert buf.data_ptr() % 256 == 0, f"the allocator returned a base that is not 256-byte aligned: {buf.data_ptr():#x}"
    buf[:pad].fill_(band)
    buf[pad:pad + nbytes].fill_(interior)
    buf[pad + nbytes:].fill_(band)
    view = buf[pad:pad + nbytes]
    assert view.numel() == nbytes and (nbytes == 0 or view.data_ptr() % 256 == 0)

    def check(what=""):
        torch.cuda.synchronize()
        hi = _damage(buf[pad + nbytes:], band)
        lo = _damage(buf[:pad], band)
        msgs = []
        if hi is not None:
            msgs.append(f"bytes BEHIND the workspace were overwritten: first at end+{hi[0]}, last at end+{hi[1]}")
        if lo is not None:
            msgs.append(f"bytes IN FRONT OF the workspace were overwritten: first at end{lo[0] - pad - nbytes}, last at "
                        f"end{lo[1] - pad - nbytes} (the workspace starts at end-{nbytes})")
        assert not msgs, f"{what}: workspace of {nbytes} bytes: " + "; ".join(msgs)

    return view, check


def roomy(nbytes, device="cuda"):
    """a workspace with generous slack whose every byte is finite as bf16 and as fp32 (what an earlier test's run leaves behind)"""
    return torch.full((2 * int(nbytes) + MIB,), FINITE, dtype=torch.uint8, device=device)


@contextlib.contextmanager
def eval_workspace(ctx, nbytes, **kw):
    """Eval paths (CNN2D, CNN1D, ConvAutoencoder, DeepfakeDetector; uniform and ragged): for the duration, the context's
    workspace is a banded view of exactly `nbytes` bytes -- what the matching planner returns for the context's CURRENT options
    (model_cae.py asks for max(planner, 256): size the view the same way).  Yields check()."""
    view, check = banded(nbytes, device=torch.device("cuda", ctx.index), **kw)
    old = ctx._ws
    ctx._ws = view
    try:
        yield check
        assert ctx._ws is view, f"the library replaced the injected workspace of {nbytes} bytes: its planner asked for more"
    finally:
        ctx._ws = old


@contextlib.contextmanager
def train_workspace(model, nbytes, **kw):
    """Training paths (forward_train_raw / backward_raw, the autograd bridge, NativeTrainer, CaeNativeTrainer, DlqTrainer): for
    the duration, model._train_ws is a banded view of exactly `nbytes` bytes.  Yields check()."""
    dev = next(model.parameters()).device
    view, check = banded(nbytes, device=dev, **kw)
    old = model.__dict__.get("_train_ws")
    model._train_ws = view
    try:
        yield check
        assert model._train_ws is view, f"the library replaced the injected training workspace of {nbytes} bytes: its planner asked for more"
    finally:
        model._train_ws = old
