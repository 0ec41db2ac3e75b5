"""The workspace planners of the C ABI on the host, over the case grid of tests/test_workspace_bounds_gpu.py: every planner that
accepts a null context is asked for each (B, T, F) of that grid and must answer with a non-zero multiple of 256 that never shrinks
when the batch or the frame count grows, and a ragged plan must cover the uniform one of the same (B, T_max, F).

Which planners read the context.  Read in deep-fake-audio-classifier_amd/csrc/*_api.hip: dfa_cae_ragged_workspace_bytes, dfa_dlq_workspace_bytes and the five
dfa_*_train*_workspace_bytes ignore it ((void)ctx): a null context exercises them completely.  dfa_workspace_bytes and
dfa_ragged_workspace_bytes (api.hip) hand it to the model's planner, and only the CNN2D's reads it (cnn2d_api.hip: the byte count
of cnn2d_forward_plan, in which ONE of the context's options counts, "time_split"; a null context plans with the defaults, so
-1): with a null context they give the automatic plan, which reserves the chunk slabs of a split time axis for small batches only
(every field of that plan: tests/test_cnn2d_plan_cpu.py).  The plan of a
FORCED split (time_split > 0 on a large batch) needs a live context and is therefore exercised on the GPU only
(test_workspace_bounds_gpu.py, test_train_shapes_gpu.py::test_forced_time_split_at_full_batch_stays_inside_the_workspace).

One documented exception to "ragged >= uniform": the ragged CNN1D forward keeps every activation in LDS, so its plan is the
per-call table alone (2 * B int32 words, include/dfa_hip.h) and is SMALLER than the uniform plan's h1 / h2 regions, which only the
three-launch uniform path uses.  It is held to its own statement instead."""
import itertools

import pytest

CNN2D_GRID = [(1, 4, 180), (2, 5, 180), (5, 33, 65), (2, 33, 5), (3, 130, 36), (2, 323, 180), (33, 7, 180), (86, 33, 180), (256, 33, 180),
              (5, 37, 180), (5, 37, 65), (3, 21, 65)]
CNN1D_GRID = [(2, 1, 180), (2, 3, 4), (3, 33, 8), (4, 100, 44), (2, 384, 180), (2, 385, 180), (5, 385, 180), (2, 37, 180), (4, 40, 180)]
CAE_GRID = [(1, 16, 20), (3, 17, 36), (2, 31, 20), (5, 70, 180), (2, 322, 180), (3, 96, 180), (5, 48, 36), (2, 17, 20)]
DLQ_GRID = [(1, 63, 180), (1, 64, 180), (1, 65, 180), (1, 132, 180), (3, 65, 180), (5, 130, 180), (3, 100, 180), (2, 5, 8)]


@pytest.fixture(scope="module")
def abi():
    from dfa_amd import _lib
    return _lib, _lib.load()


def _planners(L, lib):
    """name -> (planner(B, T, F) with a null context, grid, ragged twin's name or None)"""
    P = {}
    for pname, prec in (("fp32", L.PREC_F32), ("bf16", L.PREC_BF16), ("bf16x3", L.PREC_BF16X3)):
        P[f"cnn2d {pname}"] = (lambda B, T, F, p=prec: lib.dfa_workspace_bytes(None, L.MODEL_CNN2D, B, T, F, p), CNN2D_GRID, f"cnn2d ragged {pname}")
        P[f"cnn2d ragged {pname}"] = (lambda B, T, F, p=prec: lib.dfa_ragged_workspace_bytes(None, L.MODEL_CNN2D, B, T, F, p), CNN2D_GRID, None)
    for pname, prec in (("fp32", L.PREC_F32), ("bf16", L.PREC_BF16)):
        P[f"cnn2d train {pname}"] = (lambda B, T, F, p=prec: lib.dfa_cnn2d_train_workspace_bytes(None, B, T, F, p), CNN2D_GRID, None)
        P[f"cae {pname}"] = (lambda B, T, F, p=prec: lib.dfa_workspace_bytes(None, L.MODEL_CAE, B, T, F, p), CAE_GRID, f"cae ragged {pname}")
        P[f"cae ragged {pname}"] = (lambda B, T, F, p=prec: lib.dfa_cae_ragged_workspace_bytes(None, B, T, F, p), CAE_GRID, None)
        P[f"cae train {pname}"] = (lambda B, T, F, p=prec: lib.dfa_cae_train_workspace_bytes(None, B, T, F, p), CAE_GRID, None)
    P["cnn1d"] = (lambda B, T, F: lib.dfa_workspace_bytes(None, L.MODEL_CNN1D, B, T, F, L.PREC_F32), CNN1D_GRID, None)
    P["cnn1d train"] = (lambda B, T, F: lib.dfa_cnn1d_train_workspace_bytes(None, B, T, F), CNN1D_GRID, "cnn1d train ragged")
    P["cnn1d train ragged"] = (lambda B, T, F: lib.dfa_cnn1d_train_ragged_workspace_bytes(None, B, T, F),
                               [c for c in CNN1D_GRID if c[1] >= 3], None)
    P["dlq"] = (lambda B, T, F: lib.dfa_dlq_workspace_bytes(None, B, T, F), DLQ_GRID, None)
    P["dlq train"] = (lambda B, T, F: lib.dfa_dlq_train_workspace_bytes(None, B, T, F), DLQ_GRID, None)
    return P


def test_every_plan_is_a_nonzero_multiple_of_256(abi):
    L, lib = abi
    for name, (plan, grid, _) in _planners(L, lib).items():
        for B, T, F in grid:
            n = plan(B, T, F)
            assert n > 0 and n % 256 == 0, (name, (B, T, F), n)


def test_no_plan_shrinks_when_the_batch_or_the_frame_count_grows(abi):
    """At every case of the grid one more utterance, or one more frame, never lowers the byte count; and of two cases of the
    grid that differ in B alone, or in T alone, the larger one never has the smaller plan.

    (This is a statement about the grid, not about every pair of shapes.  The eval plan of the CNN2D reserves four chunk slabs
    of partial embeddings while B * ceil(F / 32) < 512 and drops them from there on -- the time axis is no longer split -- so
    across that one threshold a larger batch can have the SMALLER plan: at [B, 33, 180] in fp32, 101 MB for B = 85 and 71 MB for
    B = 86.  The ABI sizes a workspace per call, and a workspace too small for a call is refused, never
    overrun: test_workspace_bounds_gpu.py.)"""
    L, lib = abi
    for name, (plan, grid, _) in _planners(L, lib).items():
        for B, T, F in grid:
            n = plan(B, T, F)
            assert plan(B + 1, T, F) >= n, (name, (B, T, F), "B + 1", plan(B + 1, T, F), n)
            assert plan(B, T + 1, F) >= n, (name, (B, T, F), "T + 1", plan(B, T + 1, F), n)
        for (B0, T0, F0), (B1, T1, F1) in itertools.permutations(grid, 2):
            if F0 == F1 and ((T0 == T1 and B0 < B1) or (B0 == B1 and T0 < T1)):
                assert plan(B0, T0, F0) <= plan(B1, T1, F1), (name, (B0, T0, F0), (B1, T1, F1))


def test_a_ragged_plan_covers_the_uniform_plan(abi):
    L, lib = abi
    P = _planners(L, lib)
    pairs = 0
    for name, (plan, grid, twin) in P.items():
        if twin is None:
            continue
        ragged, rgrid, _ = P[twin]
        for B, T, F in grid:
            if (B, T, F) in rgrid:
                assert ragged(B, T, F) >= plan(B, T, F), (twin, (B, T, F), ragged(B, T, F), plan(B, T, F))
                pairs += 1
    assert pairs >= 3 * len(CNN2D_GRID) + 2 * len(CAE_GRID) + 1
    # the ragged CNN1D forward: the table alone (see the module's docstring), exactly as include/dfa_hip.h states it
    for B, T, F in CNN1D_GRID:
        if T >= 3:
            n = lib.dfa_ragged_workspace_bytes(None, L.MODEL_CNN1D, B, T, F, L.PREC_F32)
            assert n == -(-2 * B * 4 // 256) * 256 and n >= 2 * B * 4, (B, T, F, n)
    # ... and the shared ragged planner has no auto-encoder plan: 0, callers test for that value
    assert lib.dfa_ragged_workspace_bytes(None, L.MODEL_CAE, 3, 17, 36, L.PREC_BF16) == 0
