"""A/B two builds of the library (separate processes, alternating): DFA_LIB=<file name under lib/>; DFA_AB_MODE=train times the
bf16 training step instead of the eval forward, DFA_AB_MODE=train1d the CNN1D's (fp32) uniform training step, DFA_AB_MODE=caetrain the auto-encoder's bf16 training step at [256, 321, 180], DFA_AB_MODE=dlqtrain the DeepfakeDetector's training step at [256, 180, 321] with lengths in [161, 321], DFA_AB_MODE=cae the auto-encoder's bf16 anomaly score (ConvAutoencoder.score,
z-score fused) at [256, 321, 180].  The eval forward runs at [DFA_AB_B, 321, 180] (default 256) and prints the median round's
ms per call, its timing slots 0-3 and a checksum of the logits."""
import os, sys, time, torch
sys.path.insert(0, os.getcwd())
from dfa_amd import _lib
name = os.environ.get("DFA_LIB")
if name:
    _lib.LIB_PATH = os.path.join(os.path.dirname(_lib.LIB_PATH), name)
    import ctypes
    probe = ctypes.CDLL(_lib.LIB_PATH)
    _lib.SYMBOLS[:] = [s for s in _lib.SYMBOLS if hasattr(probe, s[0])]   # an older build lacks the newer entry points
import bench
if os.environ.get("DFA_AB_MODE") == "train":
    from dfa_amd.model import CNN2D
    from dfa_amd.training.train_step import NativeTrainer
    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(1)
    x = (torch.randn(256, 180, 321, generator=g) * 3.2 - 0.07).to(dev, dtype=torch.bfloat16).transpose(1, 2)
    y = (torch.rand(256, generator=g) > 0.5).float().to(dev)
    torch.manual_seed(0)
    tr = NativeTrainer(CNN2D(dropout=0.2, precision="bf16").to(dev), label_smoothing=0.05,
                       lr=float(os.environ.get("DFA_AB_LR", "1e-6")))   # tiny lr: both builds time the same activation regime
    losses = [float(tr.step(x, y)) for _ in range(5)]
    res = []
    for rnd in range(5):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        for _ in range(10): last = tr.step(x, y)
        torch.cuda.synchronize(); res.append((time.perf_counter() - t0) / 10 * 1e3)
    print(name, "train step ms median %.3f min %.3f" % (sorted(res)[2], min(res)),
          "losses", ["%.4f" % v for v in losses], "last %.4f" % float(last), flush=True)
    sys.exit(0)
if os.environ.get("DFA_AB_MODE") == "train1d":
    from dfa_amd.model_cnn1d import CNN1D
    from dfa_amd.training.train_step import NativeTrainer
    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(1)
    x = (torch.randn(256, 180, 321, generator=g) * 3.2 - 0.07).to(dev).transpose(1, 2)
    y = (torch.rand(256, generator=g) > 0.5).float().to(dev)
    torch.manual_seed(0)
    tr = NativeTrainer(CNN1D(dropout=0.2).to(dev), label_smoothing=0.05, lr=1e-6)
    losses = [float(tr.step(x, y)) for _ in range(5)]
    res = []
    for rnd in range(7):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        for _ in range(40): last = tr.step(x, y)
        torch.cuda.synchronize(); res.append((time.perf_counter() - t0) / 40 * 1e3)
    print(name, "cnn1d train step ms median %.4f min %.4f max %.4f" % (sorted(res)[3], min(res), max(res)),
          "losses", ["%.6f" % v for v in losses], "last %.6f" % float(last), flush=True)
    sys.exit(0)
if os.environ.get("DFA_AB_MODE") == "caetrain":
    from dfa_amd.model_cae import ConvAutoencoder
    from dfa_amd.training.train_step import make_cae_trainer
    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(1)
    x = torch.randn(256, 321, 180, generator=g).to(dev, torch.bfloat16)
    torch.manual_seed(0)
    tr = make_cae_trainer(ConvAutoencoder(precision="bf16").to(dev), lr=1e-6, weight_decay=1e-4)
    losses = [float(tr.step(x)) for _ in range(5)]
    res = []
    for rnd in range(5):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        for _ in range(10): last = tr.step(x)
        torch.cuda.synchronize(); res.append((time.perf_counter() - t0) / 10 * 1e3)
    print(name, "cae train step ms median %.3f min %.3f" % (sorted(res)[2], min(res)),
          "losses", ["%.6f" % v for v in losses], "last %.6f" % float(last), flush=True)
    sys.exit(0)
if os.environ.get("DFA_AB_MODE") == "dlqtrain":
    from dfa_amd.dlqueen_model import DeepfakeDetector
    from dfa_amd.training import DlqTrainer
    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(1)
    x = (torch.randn((256, 180, 324), generator=g) * 3.2 - 0.07)[:, :, :321]
    lengths = torch.randint(161, 322, (256,), generator=g)
    lengths[0] = 321
    for b in range(256): x[b, :, int(lengths[b]):] = 0.0
    y = (torch.rand(256, generator=g) > 0.5).float().to(dev)
    x, lens = x.to(dev), lengths.numpy()
    torch.manual_seed(0)
    tr = DlqTrainer(DeepfakeDetector(180, dropout=0.3).to(dev), lr=1e-6, weight_decay=1e-4, pos_weight=2.5, grad_clip=5.0, ema_decay=0.999)
    losses = [float(tr.step(x, lens, y)) for _ in range(5)]
    res = []
    for rnd in range(5):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        for _ in range(10): last = tr.step(x, lens, y)
        torch.cuda.synchronize(); res.append((time.perf_counter() - t0) / 10 * 1e3)
    print(name, "dlq train step ms median %.3f min %.3f" % (sorted(res)[2], min(res)),
          "losses", ["%.6f" % v for v in losses], "last %.6f" % float(last), flush=True)
    sys.exit(0)
if os.environ.get("DFA_AB_MODE") == "cae":
    from dfa_amd.model_cae import ConvAutoencoder
    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(1234)
    x = (torch.randn(256, 180, 321, generator=g) * 3.2 - 0.07).to(device=dev, dtype=torch.bfloat16).transpose(1, 2)
    mean, std = torch.randn(180, generator=g).to(dev), (torch.rand(180, generator=g) + 0.5).to(dev)
    torch.manual_seed(0)
    model = ConvAutoencoder(precision="bf16").to(dev).eval()
    ctx = _lib.Context.get(dev)
    for _ in range(10): last = model.score(x, mean, std)
    out = []
    for rnd in range(5):
        ctx.timing_reset(); ctx.timing(True)
        torch.cuda.synchronize(); t0 = time.perf_counter()
        for _ in range(20): last = model.score(x, mean, std)
        torch.cuda.synchronize(); dt = (time.perf_counter() - t0) / 20
        ctx.timing(False)
        sl = [ctx.timing_read(s) for s in range(8, 13)]
        out.append((round(dt * 1e3, 4), [round(ms / max(n, 1), 4) for ms, n in sl]))
    ms = sorted(o[0] for o in out)
    print(name, "cae score ms median %.4f min %.4f max %.4f" % (ms[2], ms[0], ms[-1]), "slots 8-12 of the median round", sorted(out)[2][1],
          "checksum %.9g" % float(last.double().sum()), flush=True)
    sys.exit(0)
dev = torch.device("cuda", 0)
g = torch.Generator().manual_seed(1234)
PREC = os.environ.get("DFA_AB_PREC", "bf16")
B = int(os.environ.get("DFA_AB_B", "256"))     # eval forward: the batch size ([B, 321, 180]; 1 = the host's time per call shows)
x = (torch.randn(B, 180, 321, generator=g) * 3.2 - 0.07).to(device=dev, dtype=torch.bfloat16 if PREC == "bf16" else torch.float32).transpose(1, 2)
ctx = _lib.Context.get(dev)
model = bench.build_model(torch, dev, PREC)
for _ in range(10): model(x)
out = []
for rnd in range(5):
    ctx.timing_reset(); ctx.timing(True)
    torch.cuda.synchronize(); t0 = time.perf_counter()
    for _ in range(20): model(x)
    torch.cuda.synchronize(); dt = (time.perf_counter() - t0) / 20
    ctx.timing(False)
    sl = [ctx.timing_read(s) for s in range(4)]
    out.append((round(dt * 1e3, 4), [round(ms / max(n, 1), 4) for ms, n in sl]))
print(name, "B", B, sorted(out)[len(out)//2], "checksum %.9g" % float(model(x).double().sum()), flush=True)
