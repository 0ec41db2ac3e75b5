"""The numpy statement of the two embedding anomaly scores (include/dfa_hip.h, embedding anomaly detectors), from the fitted arrays
alone -- no sklearn.  In float64 it is the oracle of every parity test; the same statement in float32 gives the error a plain fp32
evaluation makes on the same inputs, which the GPU tolerance is stated against.

A detector is a mapping of arrays: mean[D], inv_scale[D]; sv[n_sv][D], dual_coef[n_sv], gamma, intercept; pca_mean[D],
components[P][D], means[K][P], prec_chol[K][P][P], log_const[K]."""
import numpy as np

FLOOR = 2.0 ** -22          # two fp32 ulps of the result
FACTOR = 4.0


def _f(d, key, dt):
    return np.asarray(d[key]).astype(dt)


def scaled(d, emb, dt=np.float64):
    return (np.asarray(emb).astype(dt) - _f(d, "mean", dt)) * _f(d, "inv_scale", dt)


def ocsvm_scores(d, emb, dt=np.float64):
    """sum_i dual_coef[i] exp(-gamma |x~ - sv_i|^2) + intercept, the distance as |x~|^2 + |sv|^2 - 2 x~ . sv"""
    xs, sv = scaled(d, emb, dt), _f(d, "sv", dt)
    d2 = (xs * xs).sum(axis=1)[:, None] + (sv * sv).sum(axis=1)[None, :] - dt(2) * (xs @ sv.T)
    out = np.exp(-_f(d, "gamma", dt) * d2) @ _f(d, "dual_coef", dt) + _f(d, "intercept", dt)
    assert out.dtype == dt
    return out


def gmm_scores(d, emb, dt=np.float64):
    """z = (x~ - pca_mean) components^T, lp_k = -|(z - means[k]) prec_chol[k]|^2 / 2 + log_const[k], logsumexp over k"""
    z = (scaled(d, emb, dt) - _f(d, "pca_mean", dt)) @ _f(d, "components", dt).T
    mu, L, c = _f(d, "means", dt), _f(d, "prec_chol", dt), _f(d, "log_const", dt)
    lp = np.stack([dt(-0.5) * (((z - mu[k]) @ L[k]) ** 2).sum(axis=1) + c[k] for k in range(mu.shape[0])], axis=1)
    mx = lp.max(axis=1)
    out = mx + np.log(np.exp(lp - mx[:, None]).sum(axis=1))
    assert out.dtype == dt
    return out


def rel_err(s, s64):
    """e = max|s - s64| / max|s64|"""
    return float(np.abs(np.asarray(s, np.float64) - s64).max() / np.abs(s64).max())


def bound(d, emb, which):
    """(s64, e32, the GPU's allowance 4 max(e32, 2^-22)) of one case"""
    fn = ocsvm_scores if which == "ocsvm" else gmm_scores
    s64 = fn(d, emb, np.float64)
    e32 = rel_err(fn(d, emb, np.float32), s64)
    return s64, e32, FACTOR * max(e32, FLOOR)


def random_detectors(seed, D, n_sv, P, K):
    """Seeded detector arrays of any shape: post-ReLU-like training statistics with dead columns, a lower-triangular prec_chol
    with a positive diagonal, and gamma = 1 / D so that the exponents are O(1).  Returns (detectors, a function n -> embeddings)."""
    rng = np.random.default_rng(seed)
    base = np.maximum(rng.normal(0.3, 0.5, D), 0).astype(np.float32)
    dead = rng.choice(D, size=max(1, D // 40), replace=False)
    base[dead] = 0

    def rows(n, spread=0.4):
        x = np.maximum(base + rng.normal(0, spread, (n, D)).astype(np.float32) * (base > 0), 0).astype(np.float32)
        x[:, dead] = 0
        return x

    tr = rows(64)
    std = tr.std(axis=0)
    inv = np.where(std > 0, 1.0 / np.where(std > 0, std, 1), 1.0).astype(np.float32)
    mean = tr.mean(axis=0).astype(np.float32)
    d = {"mean": mean, "inv_scale": inv}
    d["sv"] = ((rows(n_sv) - mean) * inv).astype(np.float32)
    d["dual_coef"] = rng.uniform(0.05, 1.0, n_sv).astype(np.float32)
    d["gamma"] = np.float32(1.0 / D)
    d["intercept"] = np.float32(-0.3 * d["dual_coef"].sum())
    d["pca_mean"] = rng.normal(0, 0.05, D).astype(np.float32)
    q, _ = np.linalg.qr(rng.normal(size=(D, P)))
    d["components"] = np.ascontiguousarray(q.T).astype(np.float32)
    d["means"] = rng.normal(0, 2.0, (K, P)).astype(np.float32)
    L = np.tril(rng.normal(0, 0.05, (K, P, P)))
    i = np.arange(P)
    L[:, i, i] = rng.uniform(0.2, 0.6, (K, P))
    d["prec_chol"] = L.astype(np.float32)
    w = rng.dirichlet(np.ones(K))
    d["log_const"] = (np.log(L[:, i, i]).sum(axis=1) + np.log(w) - 0.5 * P * np.log(2 * np.pi)).astype(np.float32)
    return d, rows
