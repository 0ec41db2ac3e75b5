"""The per-utterance CMN / CVMN normalisation (src/compare_normalization.py:53-62) in float64 numpy,
written from the definition, with the inputs, the lengths and the per-row bound the tests of dfa_utt_norm share.

    mean = (1/n) sum_t x[c][t];  cmn: y = x - mean;  cvmn: y = (x - mean) / max(sqrt(sum_t (x - mean)^2 / (n - 1)), 1e-8)

The bound, per row:  |y - y64| <= 8 * 2^-24 * max|x_row| / s_row + 4 * 2^-24 * max|y64_row|,  s_row = 1 (cmn) or the float64
std (cvmn).  First term: the rounding of the mean, which every element of the row shares (8: room for an fp32 tree sum); second:
the rounding of the result.  The reference's own float32 expression on the CPU stays inside this bound on these inputs, at
most 2.7 units of its first term (2^-24 * max|x| / s) off the float64 value and at most a third of the whole bound
(test_utt_norm_cpu.py asserts the bound and prints the figures), so the bound is neither vacuous nor tighter than the reference."""
import functools

import numpy as np

HELD_FRAMES = 1024                    # DFA_UTT_NORM_HELD_FRAMES: the time-fastest kernel's on-chip row cap
LENGTHS = (2, 3, 4, 5, 63, 64, 65, 255, 256, 257, 321, HELD_FRAMES + 1)
CHANNELS = (4, 180)
MU_SIGMA = ((0.0, 1.0), (-20.0, 3.0), (100.0, 0.5))
MODES = ("cmn", "cvmn")
FIXTURE_LENGTHS = (2, 5, 65, 257)     # tests/golden/utt_norm.npz: [180, T] utterances through the reference's NormalizedDataset
EPS = 2.0 ** -24
STD_FLOOR = 1e-8


@functools.lru_cache(maxsize=None)
def utterance(C, T, seed=0):
    """[C, T] float32, read-only: row c is randn * sigma + mu with (mu, sigma) = MU_SIGMA[c % 3], rounded to float32"""
    rng = np.random.default_rng([17, int(C), int(T), int(seed)])
    mu = np.array([MU_SIGMA[c % 3][0] for c in range(C)])[:, None]
    sigma = np.array([MU_SIGMA[c % 3][1] for c in range(C)])[:, None]
    x = (rng.standard_normal((C, T)) * sigma + mu).astype(np.float32)
    x.setflags(write=False)
    return x


def stats(x):
    """(mean [C, 1], std [C, 1]) of a [C, n] utterance in float64: two passes, the std unbiased (n = 1: std = 0)"""
    x = np.asarray(x, dtype=np.float64)
    n = x.shape[1]
    mean = x.sum(axis=1, keepdims=True) / n
    css = ((x - mean) ** 2).sum(axis=1, keepdims=True)
    return mean, np.sqrt(css / max(n - 1, 1))


def normalize(x, mode):
    """float64 [C, n] of a float32 [C, n] utterance"""
    if mode not in MODES:
        raise ValueError(mode)
    mean, std = stats(x)
    d = np.asarray(x, dtype=np.float64) - mean
    return d if mode == "cmn" else d / np.maximum(std, STD_FLOOR)


def first_term(x, mode):
    """2^-24 * max|x_row| / s_row, [C]: the unit of the bound's first term"""
    _, std = stats(x)
    s = np.ones(x.shape[0]) if mode == "cmn" else np.maximum(std[:, 0], STD_FLOOR)
    return EPS * np.abs(np.asarray(x, dtype=np.float64)).max(axis=1) / s


def row_bound(x, mode):
    """[C]: 8 * 2^-24 * max|x_row| / s_row + 4 * 2^-24 * max|y64_row|"""
    return 8.0 * first_term(x, mode) + 4.0 * EPS * np.abs(normalize(x, mode)).max(axis=1)


@functools.lru_cache(maxsize=None)
def expected(C, T, mode, seed=0):
    """(y64 [C, T], bound [C]) of utterance(C, T, seed), computed once and read-only"""
    x = utterance(C, T, seed)
    y, b = normalize(x, mode), row_bound(x, mode)
    y.setflags(write=False)
    b.setflags(write=False)
    return y, b


def reference32(x, mode):
    """the reference's own expression (NormalizedDataset.__getitem__) in float32 torch on the CPU -> numpy [C, n]"""
    import torch
    feat = torch.from_numpy(np.array(x, dtype=np.float32))
    if mode == "cmn":
        feat = feat - feat.mean(dim=1, keepdim=True)
    else:
        mean = feat.mean(dim=1, keepdim=True)
        std = feat.std(dim=1, keepdim=True).clamp(min=1e-8)
        feat = (feat - mean) / std
    return feat.numpy()
