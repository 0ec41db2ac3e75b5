"""CPU side of the embedding anomaly detectors: the C ABI table, the numpy statement of the two scores (tests/emb_oracle.py) against
what sklearn itself computed (tests/golden/emb_detectors.npz, written by tests/golden/make_golden_emb.py), the host fit against
sklearn where sklearn is installed, the Detectors file, and the command line."""
import importlib.util
import os
import re

import numpy as np
import pytest

import emb_oracle as EO
from dfa_amd import _lib, embedding_anomaly as EA
from dfa_amd.evaluation import calculate_eer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("dfa_emb_ocsvm_bind", "dfa_emb_gmm_bind", "dfa_emb_workspace_bytes", "dfa_emb_ocsvm_score", "dfa_emb_gmm_score")
DET_KEYS = ("mean", "inv_scale", "sv", "dual_coef", "gamma", "intercept", "pca_mean", "components", "means", "prec_chol", "log_const")


@pytest.fixture(scope="module")
def fx():
    with np.load(os.path.join(ROOT, "tests", "golden", "emb_detectors.npz")) as z:
        return {k: z[k] for k in z.files}


def _generator():
    spec = importlib.util.spec_from_file_location("make_golden_emb", os.path.join(ROOT, "tests", "golden", "make_golden_emb.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_library_exports_the_new_symbols_and_the_limits():
    lib = _lib.load()
    bound = {n for n, _, _ in _lib.SYMBOLS}
    header = open(os.path.join(ROOT, "include", "dfa_hip.h")).read()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name) and name in bound, name
        assert re.search(r"\b%s\s*\(" % name, header), name
    for macro, value in (("DFA_EMB_OCSVM", _lib.EMB_OCSVM), ("DFA_EMB_GMM", _lib.EMB_GMM), ("DFA_EMB_MAX_P", _lib.EMB_MAX_P),
                         ("DFA_EMB_MAX_K", _lib.EMB_MAX_K)):
        assert int(re.search(r"#define %s (\d+)" % macro, header).group(1)) == value
    ws = lib.dfa_emb_workspace_bytes
    assert ws(_lib.EMB_OCSVM, 3, 640, 65, 0) % 256 == 0 and ws(_lib.EMB_OCSVM, 3, 640, 65, 0) >= 3 * 65 * 4
    assert ws(_lib.EMB_GMM, 3, 640, 32, 4) >= 3 * 32 * 4 * (1 + 1 + 4)
    for bad in ((_lib.EMB_OCSVM, 0, 640, 65, 0), (_lib.EMB_OCSVM, 3, 100, 65, 0), (_lib.EMB_OCSVM, 3, 640, 0, 0), (_lib.EMB_GMM, 3, 640, 257, 4),
                (_lib.EMB_GMM, 3, 640, 0, 4), (_lib.EMB_GMM, 3, 640, 32, 0), (_lib.EMB_GMM, 3, 640, 32, 65), (2, 3, 640, 32, 4)):
        assert ws(*bad) == 0, bad
    # the split of the long reduction is a rule of D and the column count: the planner is linear in N
    assert ws(_lib.EMB_OCSVM, 256, 23040, 2000, 0) == 2 * ws(_lib.EMB_OCSVM, 128, 23040, 2000, 0)


def test_fixture_shapes_and_dead_columns(fx):
    D, n_sv, P, K = 640, fx["sv"].shape[0], 32, 4
    assert fx["dev"].shape == (100, D) and fx["dev"].dtype == np.float32 and (fx["dev"] >= 0).all()
    assert fx["components"].shape == (P, D) and fx["prec_chol"].shape == (K, P, P) and fx["means"].shape == (K, P) and n_sv >= 10
    assert set(fx["labels"].tolist()) == {0.0, 1.0}
    dead = fx["inv_scale"] == 1.0
    assert dead.sum() == 12 and (fx["dev"][:, dead] == 0).all()          # zero-variance columns: sklearn's scale_ = 1
    assert all(fx[k].dtype == np.float32 for k in DET_KEYS)


def test_float64_statement_reproduces_the_recorded_sklearn_scores(fx):
    for fn, key in ((EO.ocsvm_scores, "sklearn_ocsvm"), (EO.gmm_scores, "sklearn_gmm")):
        s64 = fn(fx, fx["dev"], np.float64)
        assert np.abs(s64 - fx[key]).max() <= 1e-4 * np.abs(fx[key]).max(), key
        e64 = calculate_eer(s64.tolist(), fx["labels"].tolist())
        e32 = calculate_eer(fn(fx, fx["dev"], np.float32).astype(np.float64).tolist(), fx["labels"].tolist())
        assert e64[0] == e32[0] == calculate_eer(fx[key].tolist(), fx["labels"].tolist())[0] and 0.0 < e64[0] < 0.5


def test_random_detectors_are_what_the_gpu_tests_assume():
    d, rows = EO.random_detectors(3, 128, 33, 7, 3)
    x = rows(5)
    assert (np.triu(d["prec_chol"], 1) == 0).all() and (np.diagonal(d["prec_chol"], axis1=1, axis2=2) > 0).all()
    assert (d["inv_scale"] == 1).sum() >= 1 and x.dtype == np.float32 and (x >= 0).all()
    expo = float(d["gamma"]) * ((EO.scaled(d, x)[:, None, :] - d["sv"][None].astype(np.float64)) ** 2).sum(axis=2)
    assert 0.05 < expo.min() and expo.max() < 50                      # exponents of order one
    for which in ("ocsvm", "gmm"):
        s64, e32, tol = EO.bound(d, x, which)
        assert np.isfinite(s64).all() and tol >= 4 * EO.FLOOR and e32 < 1e-5


def test_fit_detectors_reproduces_sklearn(fx):
    pytest.importorskip("sklearn")
    gen = _generator()
    train, dev, labels = gen.recipe()
    np.testing.assert_array_equal(dev, fx["dev"])
    det_sk, sk_svm, sk_gmm = gen.sklearn_scores(train, dev)
    det = EA.fit_detectors(train[:, :], gmm_components=4)               # PCA: min(256, 640, 200) = 200 components here
    assert det.dims == (640, det_sk["sv"].shape[0], 200, 4)
    assert float(det.gamma) == float(det_sk["gamma"])                    # 'scale', as sklearn resolves it
    dead = train.std(axis=0) == 0
    assert dead.sum() == gen.DEAD and (det.inv_scale[dead] == 1).all() and (det.inv_scale[~dead] != 1).all()
    s = EO.ocsvm_scores(det, dev)
    assert np.abs(s - sk_svm).max() <= 1e-4 * np.abs(sk_svm).max()
    # the mixture on all 200 principal components: against sklearn's own calls on the same fit
    from sklearn.decomposition import PCA
    from sklearn.mixture import GaussianMixture
    from sklearn.preprocessing import StandardScaler
    sc = StandardScaler().fit(train)
    pca = PCA(n_components=200, random_state=42)
    gm = GaussianMixture(n_components=4, covariance_type="full", reg_covar=1e-4, random_state=42).fit(pca.fit_transform(sc.transform(train)))
    want = gm.score_samples(pca.transform(sc.transform(dev)))
    got = EO.gmm_scores(det, dev)
    assert np.abs(got - want).max() <= 1e-4 * np.abs(want).max()


def test_detectors_file_roundtrips_bit_for_bit(fx, tmp_path):
    det = EA.Detectors(**{k: fx[k] for k in DET_KEYS})
    assert det.dims == (640, fx["sv"].shape[0], 32, 4)
    path = str(tmp_path / "det.npz")
    det.save(path)
    back = EA.Detectors.load(path)
    for k in DET_KEYS:
        a, b = getattr(det, k), getattr(back, k)
        assert a.dtype == b.dtype == np.float32 and a.shape == b.shape and a.tobytes() == b.tobytes(), k
    with np.load(path, allow_pickle=False) as z:
        assert sorted(z.files) == sorted(DET_KEYS)                        # arrays only
    np.savez(str(tmp_path / "short.npz"), mean=fx["mean"])
    with pytest.raises(ValueError, match="lacks"):
        EA.Detectors.load(str(tmp_path / "short.npz"))
    with pytest.raises(ValueError, match="prec_chol"):
        EA.Detectors(**{**{k: fx[k] for k in DET_KEYS}, "prec_chol": fx["prec_chol"][:, :, :5]})


def test_parser_has_the_reference_defaults():
    a = EA.parse_args(["--checkpoint", "c.pt"])
    assert (a.checkpoint, a.train_features, a.train_labels, a.dev_features, a.dev_labels) == \
        ("c.pt", "data/train/features.pkl", "data/train/labels.pkl", "data/dev/features.pkl", "data/dev/labels.pkl")
    assert (a.batch_size, a.device, a.in_features, a.dropout, a.swap_tf, a.gmm_components, a.svm_nu, a.svm_kernel) == \
        (32, None, 180, 0.2, True, 8, 0.05, "rbf")
    assert (a.precision, a.save_detectors, a.detectors, a.out, a.score) == ("fp32", None, None, None, "ocsvm")
    assert EA.parse_args(["--checkpoint", "c.pt", "--no-swap-tf"]).swap_tf is False
    with pytest.raises(SystemExit):
        EA.parse_args([])


def test_other_svm_kernels_are_refused_by_name(capsys):
    with pytest.raises(SystemExit) as e:
        EA.parse_args(["--checkpoint", "c.pt", "--svm-kernel", "linear"])
    assert e.value.code != 0 and "linear" in capsys.readouterr().err
    with pytest.raises(ValueError, match="'linear'.*no CPU fallback"):
        EA.fit_detectors(np.zeros((4, 128), np.float32), svm_kernel="linear")


def test_scorer_has_no_cpu_path(fx):
    det = EA.Detectors(**{k: fx[k] for k in DET_KEYS})
    with pytest.raises(RuntimeError, match="GPU only"):
        EA.EmbeddingScorer(det, "cpu")
