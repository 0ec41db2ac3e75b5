"""norm= in the host-fed loops (Wiring): every loop normalises its batch where it reaches the device,
before the augmentation and the model.  Each comparison repeats the loop's own steps by hand -- normalization.normalize_batch /
normalize_stored in front of the same call on the same layout, on a twin model with the same seeds -- so it is exact; that the
normalisation itself is right is tests/test_utt_norm_gpu.py's matter."""
import random

import numpy as np
import pytest
import torch

import utt_norm_oracle as UO

pytestmark = pytest.mark.gpu
F, T = 180, 321


def _utts(lens, seed, Cc=F):
    return [torch.from_numpy(np.array(UO.utterance(Cc, n, seed=seed))) for n in lens]


def _cnn1d(seed=5):
    from dfa_amd.model_cnn1d import CNN1D
    torch.manual_seed(seed)
    m = CNN1D(in_features=F, dropout=0.2).to("cuda")
    m._drop_seed, m._drop_offset = 77, 0
    return m


@pytest.mark.parametrize("mode", UO.MODES)
def test_dlqueen_host_loop_equals_the_resident_set(mode):
    """epoch_batches(norm=) builds the batches DlqResidentSet(norm=) gathers (normalised, then masked), run_inference(norm=) gives
    the scores of the resident file-order pass, bit for bit"""
    from dfa_amd.dataloaders import DlqResidentSet
    from dfa_amd.dlqueen_model import DeepfakeDetector, run_inference, run_inference_resident
    from dfa_amd.train_dlqueen import epoch_batches, resident_epoch_batches
    Cc = 12
    lens = [9, 65, 2, 130, 33, 257, 64]
    feats = _utts(lens, 11, Cc)
    labels = np.array([i % 2 for i in range(len(lens))])
    order = [3, 0, 5, 5, 2, 6, 1, 4]
    specaug = (30, 2, 5, 2)
    rset = DlqResidentSet(feats, labels, device="cuda", norm=mode)
    host = epoch_batches(feats, labels, order, 3, specaug, random.Random(4), norm=mode, device="cuda")
    res = resident_epoch_batches(rset, order, 3, specaug, random.Random(4))
    n = 0
    for (x, ln, y), (xr, lnr, yr) in zip(host, res):
        assert x.is_cuda and np.array_equal(ln, lnr) and torch.equal(y.to("cuda"), yr)
        assert torch.equal(x.contiguous().view(torch.int32), xr.contiguous().view(torch.int32))
        n += 1
    assert n == 3
    with pytest.raises(ValueError, match="device"):
        next(epoch_batches(feats, labels, order, 3, norm=mode))
    torch.manual_seed(2)
    model = DeepfakeDetector(in_ch=Cc).to("cuda").eval()
    want = run_inference_resident(model, rset, batch_size=3)
    assert torch.equal(run_inference(model, feats, 3, device="cuda", file_order=True, norm=mode), want)
    sorted_batches = run_inference(model, feats, 3, device="cuda", norm=mode)
    raw = run_inference(model, feats, 3, device="cuda")
    assert sorted_batches.shape == want.shape and not torch.equal(sorted_batches, raw)


@pytest.mark.parametrize("mode", UO.MODES)
def test_evaluate_loops_normalise_each_batch(mode):
    from dfa_amd.evaluation import evaluate, evaluate_ragged, evaluate_sharded
    from dfa_amd.normalization import normalize_stored
    from dfa_amd.predict import predict_scores_ragged
    model = _cnn1d().eval()
    feats = torch.stack(_utts([T] * 5, 21))
    labels = torch.tensor([0.0, 1.0, 1.0, 0.0, 1.0])
    loader = [(feats[:3], labels[:3]), (feats[3:], labels[3:])]
    with torch.no_grad():
        want = torch.cat([model(normalize_stored(f.to("cuda"), mode).transpose(1, 2)).squeeze(-1) for f, _ in loader]).cpu().tolist()
    _, scores, labs = evaluate(model, loader, device="cuda", swap_tf=True, norm=mode)
    assert scores == want and labs == labels.tolist()
    _, scores, _ = evaluate_sharded(model, feats, labels, device="cuda", batch_size=3, norm=mode)
    assert [float(np.float32(s)) for s in scores] == want
    assert evaluate(model, loader, device="cuda", swap_tf=True)[1] != want
    utts = _utts([T, 40, 257, 64, 9], 22)
    _, scores, _ = evaluate_ragged(model, utts, labels.numpy(), device="cuda", batch_size=3, norm=mode)
    assert scores == predict_scores_ragged(model, utts, batch_size=3, device="cuda", apply_sigmoid=False, norm=mode).cpu().tolist()


@pytest.mark.parametrize("mode", UO.MODES)
def test_training_loops_normalise_each_batch(mode):
    from dfa_amd.dataloaders import RaggedBatcher
    from dfa_amd.normalization import normalize_batch, normalize_stored
    from dfa_amd.train import make_criterion, train_one_epoch, train_one_epoch_native, train_one_epoch_ragged
    from dfa_amd.training.train_step import NativeTrainer
    feats = torch.stack(_utts([T] * 4, 31))
    labels = torch.tensor([0.0, 1.0, 1.0, 0.0])
    # the autograd bridge
    a, b = _cnn1d(), _cnn1d()
    crit = make_criterion(0.05)
    loss = train_one_epoch(a, [(feats, labels)], crit, torch.optim.SGD(a.parameters(), lr=0.01), device="cuda", swap_tf=True, norm=mode)
    b.train()
    x = normalize_stored(feats.to("cuda"), mode).transpose(1, 2)
    want = crit(b(x).squeeze(-1), labels.to("cuda"))
    assert loss == float(want.detach().double().item())
    # the all-native step on stored batches
    a, b = _cnn1d(), _cnn1d()
    ta, tb = NativeTrainer(a, lr=1e-3, label_smoothing=0.05), NativeTrainer(b, lr=1e-3, label_smoothing=0.05)
    dev = [(feats.to("cuda"), labels.to("cuda"))]
    loss = train_one_epoch_native(ta, dev, None, True, norm=mode)
    want = tb.step(normalize_stored(dev[0][0], mode).transpose(1, 2), dev[0][1])
    assert loss == float(want.detach().double().squeeze().item())
    assert loss != train_one_epoch_native(NativeTrainer(_cnn1d(), lr=1e-3, label_smoothing=0.05), dev, None, True)
    # the variable-length native step
    utts = _utts([T, 40, 257, 64], 32)
    a, b = _cnn1d(), _cnn1d()
    ta, tb = NativeTrainer(a, lr=1e-3, label_smoothing=0.05), NativeTrainer(b, lr=1e-3, label_smoothing=0.05)
    loss = train_one_epoch_ragged(ta, RaggedBatcher(utts, labels.numpy(), 4, device="cuda"), norm=mode)
    (xb, yb, lb), = list(RaggedBatcher(utts, labels.numpy(), 4, device="cuda"))
    want = tb.step(normalize_batch(xb, mode, lb, out=xb), yb, lengths=lb)
    assert loss == float(want.detach().double().squeeze().item())
    for pa, pb in zip(a.parameters(), b.parameters()):
        assert torch.equal(pa, pb)
