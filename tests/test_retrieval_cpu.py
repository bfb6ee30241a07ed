"""Corpus retrieval without a GPU: the host-side plan and argument contract of ste_topk_sim
(no launch), retrieval_metrics on hand-made ranks, the ste::topk_sim op's schema and fake
shapes, and the reference logic the GPU tests rely on (np.lexsort against a brute-force loop
under ties)."""
import ctypes as C
import math

import numpy as np
import pytest
import torch
from torch._subclasses.fake_tensor import FakeTensorMode

import speech_transcript_embeddings_amd as ste
from speech_transcript_embeddings_amd import _lib, torch_ops

from retrieval_ref import brute_force_topk, lexsort_topk, ref_ranks

ERR_ARG, ERR_SHAPE = 1001, 1002
QT, CT = 32, 64   # the kernel's query / corpus tile (csrc/retrieval.hip)


def plan(Q, N, P, k, splits):
    s, b = C.c_int(-1), C.c_int64(-1)
    rc = _lib.fn("ste_topk_sim_plan")(Q, N, P, k, splits, C.byref(s), C.byref(b))
    return rc, s.value, b.value


def ws_bytes(Q, k, S):
    """Target scratch (a score and an id per query) + for S > 1 the partial lists: k values and
    k indices per (query, slice), and one rank count."""
    return Q * 8 + (Q * S * (8 * k + 4) if S > 1 else 0)


@pytest.mark.parametrize("Q,N,P,k", [(1, 1, 4, 1), (33, 1000, 256, 10), (1024, 65536, 256, 10), (70, 65, 66, 128),
                                     (4096, 1 << 20, 1024, 128), (1, 1 << 20, 64, 5)])
def test_plan_automatic(Q, N, P, k):
    rc, S, b = plan(Q, N, P, k, 0)
    ntiles = math.ceil(N / CT)
    assert rc == 0 and 1 <= S <= ntiles
    assert b == ws_bytes(Q, k, S)


def test_plan_fills_the_chip_for_few_queries():
    # one query tile against 2^20 rows: the corpus is cut so that every CU has work
    assert plan(1, 1 << 20, 64, 5, 0)[1] >= 256
    # many query tiles already fill it: no slices, no partial lists
    rc, S, b = plan(1 << 15, 4096, 64, 5, 0)
    assert (rc, S, b) == (0, 1, (1 << 15) * 8)


@pytest.mark.parametrize("splits", [1, 2, 7, 16])
def test_plan_forced_splits_honoured(splits):
    rc, S, b = plan(70, 1000, 66, 10, splits)       # 16 corpus tiles
    assert (rc, S) == (0, splits) and b == ws_bytes(70, 10, splits)


def test_plan_clamps_splits_to_corpus_tiles():
    assert plan(17, 65, 20, 10, 7)[:2] == (0, 2)    # 65 rows = 2 tiles
    assert plan(17, 5, 20, 10, 7)[:2] == (0, 1)
    assert plan(17, 5, 20, 10, 7)[2] == ws_bytes(17, 10, 1)


def test_argument_errors_before_launch():
    assert plan(8, 100, 64, 0, 0)[0] == ERR_ARG
    assert plan(8, 100, 64, 129, 0)[0] == ERR_ARG
    assert plan(8, 0, 64, 10, 0)[0] == ERR_ARG
    assert plan(0, 100, 64, 10, 0)[0] == ERR_ARG
    assert plan(8, 100, 1025, 10, 0)[0] == ERR_SHAPE
    assert plan(8, 100, 1024, 128, 0)[0] == 0
    f = _lib.fn("ste_topk_sim")
    # the same checks guard the launch path; the pointers are never dereferenced
    for k, N, P, want in [(0, 100, 64, ERR_ARG), (129, 100, 64, ERR_ARG), (10, 0, 64, ERR_ARG),
                          (10, 100, 1025, ERR_SHAPE)]:
        assert f(16, 16, 0, 8, N, P, k, 0, None, None, 0, 16, 16, None, 16, 1 << 20, None) == want
    # workspace too small, missing outputs, a target without a rank output, a negative base
    assert f(16, 16, 0, 8, 100, 64, 10, 0, None, None, 0, 16, 16, None, 16, 8, None) == ERR_ARG
    assert f(16, 16, 0, 8, 100, 64, 10, 0, None, None, 0, None, 16, None, 16, 1 << 20, None) == ERR_ARG
    assert f(16, 16, 0, 8, 100, 64, 10, 0, 16, None, 0, 16, 16, None, 16, 1 << 20, None) == ERR_ARG
    assert f(16, 16, 0, 8, 100, 64, 10, -1, None, None, 0, 16, 16, None, 16, 1 << 20, None) == ERR_ARG
    m = _lib.fn("ste_topk_merge")
    assert m(16, 16, 4, 20, 0, None, 0, 16, 16, None, None) == ERR_ARG
    assert m(16, 16, 4, 20, 129, None, 0, 16, 16, None, None) == ERR_ARG
    assert m(16, 16, 4, 20, 10, 16, 2, 16, 16, None, None) == ERR_ARG     # counts without a rank output


def test_retrieval_metrics_hand_made():
    r = torch.tensor([0, 4, 9, -1, 10, 0, -1, 99])
    m = ste.retrieval_metrics(r)
    kept = np.array([0, 4, 9, 10, 0, 99], dtype=np.float64)
    assert m["n"] == 6
    assert m["recall@1"] == pytest.approx(2 / 6) and m["recall@5"] == pytest.approx(3 / 6)
    assert m["recall@10"] == pytest.approx(4 / 6)
    assert m["mrr"] == pytest.approx(np.mean(1.0 / (kept + 1.0)))
    assert m["median_rank"] == pytest.approx(np.median(kept) + 1.0)
    assert set(m) == {"recall@1", "recall@5", "recall@10", "mrr", "median_rank", "n"}
    m2 = ste.retrieval_metrics(torch.tensor([2, 0, 1]), ks=(1, 2))
    assert m2 == {"recall@1": pytest.approx(1 / 3), "recall@2": pytest.approx(2 / 3),
                  "mrr": pytest.approx((1 / 3 + 1 + 1 / 2) / 3), "median_rank": 2.0, "n": 3}


@pytest.mark.parametrize("ranks", [torch.empty(0, dtype=torch.int64), torch.tensor([-1, -1])])
def test_retrieval_metrics_empty(ranks):
    assert ste.retrieval_metrics(ranks) == {"recall@1": 0.0, "recall@5": 0.0, "recall@10": 0.0, "mrr": 0.0,
                                            "median_rank": 0.0, "n": 0}


def test_topk_sim_op_schema_and_fake_shapes():
    assert "topk_sim" in torch_ops.OPS
    # torch.library prints an int argument of a custom op as SymInt
    s = str(torch.ops.ste.topk_sim.default._schema).replace("SymInt", "int")
    assert s == "ste::topk_sim(Tensor q, Tensor corpus, int k) -> (Tensor, Tensor)", s
    with FakeTensorMode():
        for dt in (torch.float32, torch.bfloat16):
            v, i = torch.ops.ste.topk_sim(torch.empty(33, 256), torch.empty(1000, 256, dtype=dt), 10)
            assert v.shape == (33, 10) and v.dtype == torch.float32
            assert i.shape == (33, 10) and i.dtype == torch.int32


def test_package_exports():
    for name in ("EmbeddingIndex", "retrieval_metrics", "embed_texts", "embed_audio", "evaluate_retrieval"):
        assert callable(getattr(ste, name))


def test_reference_lexsort_equals_brute_force_under_ties():
    """The GPU tests' reference (np.lexsort((index, -S))) against a selection loop that applies the
    order's definition pair by pair, on scores full of ties, with k above and below N."""
    rng = np.random.default_rng(0)
    for N, k in [(1, 3), (5, 10), (40, 1), (40, 7), (64, 64), (130, 128)]:
        S = rng.integers(-2, 3, size=(6, N)).astype(np.float64)      # 5 distinct values: ties everywhere
        S[0] = 1.0                                                   # a row of identical scores
        v, i = lexsort_topk(S, k, base=100)
        bv, bi = brute_force_topk(S, k, base=100)
        assert np.array_equal(v, bv) and np.array_equal(i, bi)
        if N >= k:
            assert np.array_equal(i[0], 100 + np.arange(k))
        else:
            assert np.all(np.isneginf(v[:, N:])) and np.all(i[:, N:] == -1)
        tgt = rng.integers(-1, N, size=6)
        want = [-1 if t < 0 else sum(1 for j in range(N) if S[r, j] > S[r, t] or (S[r, j] == S[r, t] and j < t))
                for r, t in enumerate(tgt)]
        assert ref_ranks(S, tgt).tolist() == want
