"""Writes tests/golden/emb_detectors.npz: a StandardScaler + OneClassSVM + PCA + GaussianMixture fitted with sklearn, exactly as
src/embedding_anomaly.py:129-158 fits them, on seeded synthetic embeddings that look like the CNN2D's (post-ReLU: non-negative, a
shared base pattern, a few columns that are zero in every row), at D = 640 (F = 5), 200 training rows, P = 32, K = 4 -- as plain
arrays, with about 100 dev embeddings in two differently spread groups, their 0 / 1 labels and sklearn's own two score vectors.

    python tests/golden/make_golden_emb.py

Needs sklearn; imports nothing of the reference.  Before it writes, it checks that the float32 and the float64 numpy statements
of the scores (tests/emb_oracle.py) reproduce sklearn, and give the SAME equal error rate, neither 0 nor 0.5, for both detectors:
the GPU test asserts that equality, so the inputs must be ones on which arithmetic noise alone cannot break it."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SEED, D, N_TRAIN, N_DEV, P, K = 20, 640, 200, 100, 32, 4
DEAD = 12                      # columns that are zero in every row: StandardScaler's scale_ is 1 there


def recipe(seed=SEED):
    """(train [200, 640], dev [100, 640], dev labels): the dev set's first half is drawn as the training set is (label 1), its
    second half around a slightly shifted base with a wider spread (label 0), so that the classes overlap"""
    rng = np.random.default_rng(seed)
    base = np.maximum(rng.normal(0.4, 0.6, D), 0)
    dead = rng.choice(D, size=DEAD, replace=False)
    base[dead] = 0
    shift = rng.normal(0, 0.13, D) * (base > 0)

    def rows(n, centre, spread):
        x = np.maximum(centre + rng.normal(0, spread, (n, D)) * rng.uniform(0.5, 1.5, (n, 1)), 0)
        x[:, dead] = 0
        return x.astype(np.float32)

    train = rows(N_TRAIN, base, 0.35)
    dev = np.concatenate([rows(N_DEV // 2, base, 0.35), rows(N_DEV - N_DEV // 2, base + shift, 0.42)])
    labels = np.concatenate([np.ones(N_DEV // 2), np.zeros(N_DEV - N_DEV // 2)]).astype(np.float32)
    return train, dev, labels


def sklearn_scores(train, dev, gmm_components=K, svm_nu=0.05):
    """the reference's own calls (src/embedding_anomaly.py:130-161), with PCA at P components"""
    from sklearn.decomposition import PCA
    from sklearn.mixture import GaussianMixture
    from sklearn.preprocessing import StandardScaler
    from sklearn.svm import OneClassSVM
    scaler = StandardScaler()
    tr, dv = scaler.fit_transform(train), None
    dv = scaler.transform(dev)
    ocsvm = OneClassSVM(kernel="rbf", nu=svm_nu).fit(tr)
    pca = PCA(n_components=min(P, tr.shape[1], tr.shape[0]), random_state=42)
    tp = pca.fit_transform(tr)
    gmm = GaussianMixture(n_components=gmm_components, covariance_type="full", reg_covar=1e-4, random_state=42).fit(tp)
    chol = gmm.precisions_cholesky_
    det = {"mean": scaler.mean_, "inv_scale": 1.0 / scaler.scale_, "sv": ocsvm.support_vectors_, "dual_coef": ocsvm.dual_coef_[0],
           "gamma": ocsvm._gamma, "intercept": ocsvm.intercept_[0], "pca_mean": pca.mean_, "components": pca.components_,
           "means": gmm.means_, "prec_chol": chol,
           "log_const": np.log(np.diagonal(chol, axis1=1, axis2=2)).sum(axis=1) + np.log(gmm.weights_) - 0.5 * chol.shape[1] * np.log(2 * np.pi)}
    det = {k: np.require(v, dtype=np.float32, requirements="C") for k, v in det.items()}
    return det, ocsvm.decision_function(dv), gmm.score_samples(pca.transform(dv))


def main():
    sys.path.insert(0, os.path.dirname(HERE))                       # tests/
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))      # the repository: dfa_amd
    import emb_oracle as EO
    from dfa_amd.evaluation import calculate_eer

    train, dev, labels = recipe()
    det, sk_svm, sk_gmm = sklearn_scores(train, dev)
    assert (det["inv_scale"] == 1).sum() == DEAD and det["sv"].shape[0] >= 1
    for name, fn, sk in (("ocsvm", EO.ocsvm_scores, sk_svm), ("gmm", EO.gmm_scores, sk_gmm)):
        s64, s32 = fn(det, dev, np.float64), fn(det, dev, np.float32)
        rel = np.abs(s64 - sk).max() / np.abs(sk).max()
        e64, e32 = calculate_eer(s64.tolist(), labels.tolist()), calculate_eer(s32.astype(np.float64).tolist(), labels.tolist())
        esk = calculate_eer(sk.tolist(), labels.tolist())
        print(f"{name}: n_sv={det['sv'].shape[0]} |s64 - sklearn| / max|sklearn| = {rel:.2e}, e32 = {EO.rel_err(s32, s64):.2e}, "
              f"EER float64 {e64[0]:.4f} float32 {e32[0]:.4f} sklearn {esk[0]:.4f}")
        assert rel < 1e-4, rel
        assert e64[0] == e32[0] == esk[0] and 0.0 < e64[0] < 0.5, (e64, e32, esk)
    out = os.path.join(HERE, "emb_detectors.npz")
    np.savez_compressed(out, dev=dev, labels=labels, sklearn_ocsvm=sk_svm, sklearn_gmm=sk_gmm, seed=np.int64(SEED), **det)
    print(f"wrote {out}: {os.path.getsize(out)} bytes")


if __name__ == "__main__":
    main()
