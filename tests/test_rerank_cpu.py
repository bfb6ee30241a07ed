"""Reranking without a GPU: the candidate plan, the reranked order and the reranked
rank against brute-force loops; the ste::xattn_mq schema and fake implementation; and the
argument contract of ste_xattn_mq_fwd / ste_xattn_gather_fwd, which returns before any launch."""
import pytest
import torch
from torch._subclasses.fake_tensor import FakeTensorMode

import speech_transcript_embeddings_amd as ste
from speech_transcript_embeddings_amd import torch_ops
from speech_transcript_embeddings_amd.retrieval import plan_candidates, rerank_order, reranked_ranks

NEG = float("-inf")
# duplicate ids within and across rows, -1 slots, an all-empty row
IDX = [[7, 3, 7, 9], [3, -1, 11, 3], [-1, -1, -1, -1], [0, 9, -1, 2]]


def test_names_are_exported():
    for name in ("plan_candidates", "rerank_order", "reranked_ranks", "rerank"):
        assert callable(getattr(ste, name))


@pytest.mark.parametrize("dtype", [torch.int32, torch.int64])
def test_plan_candidates_matches_loops(dtype):
    idx = torch.tensor(IDX, dtype=dtype)
    unique, slots = plan_candidates(idx)
    want = sorted({v for row in IDX for v in row if v >= 0})
    assert unique.tolist() == want and unique.dtype == dtype
    assert slots.shape == idx.shape
    for r, row in enumerate(IDX):
        for c, v in enumerate(row):
            assert slots[r, c].item() == (want.index(v) if v >= 0 else -1)


def test_plan_candidates_edges():
    unique, slots = plan_candidates(torch.tensor([[5]], dtype=torch.int32))          # k = 1
    assert unique.tolist() == [5] and slots.tolist() == [[0]]
    unique, slots = plan_candidates(torch.full((2, 3), -1, dtype=torch.int32))      # nothing retrieved
    assert unique.numel() == 0 and slots.tolist() == [[-1] * 3] * 2


def _order_loops(scores, idx):
    vals, ids = [], []
    for srow, irow in zip(scores, idx):
        live = sorted((p for p in range(len(irow)) if irow[p] >= 0), key=lambda p: (-srow[p], p))
        n_empty = len(irow) - len(live)
        vals.append([srow[p] for p in live] + [NEG] * n_empty)
        ids.append([irow[p] for p in live] + [-1] * n_empty)
    return vals, ids


def test_rerank_order_matches_loops():
    # ties (stage-1 position breaks them), a score on an empty slot that must not count, k = 4
    scores = [[0.5, 0.75, 0.5, 0.75], [0.25, 9.0, 0.25, 0.25], [1.0, 2.0, 3.0, 4.0], [-1.0, -1.0, 5.0, 0.0]]
    v, i = rerank_order(torch.tensor(scores), torch.tensor(IDX, dtype=torch.int32))
    wv, wi = _order_loops(scores, IDX)
    assert v.tolist() == wv and i.tolist() == wi and i.dtype == torch.int32
    assert i[0].tolist() == [3, 9, 7, 7] and i[1].tolist() == [3, 11, 3, -1] and i[2].tolist() == [-1] * 4
    v, i = rerank_order(torch.tensor([[0.125]]), torch.tensor([[4]]))                 # k = 1
    assert v.tolist() == [[0.125]] and i.tolist() == [[4]]
    g = torch.Generator().manual_seed(0)
    s = torch.randint(0, 4, (50, 6), generator=g).float()                            # many ties
    ids = torch.stack([torch.randperm(40, generator=g)[:6] for _ in range(50)])
    ids[torch.rand(50, 6, generator=g) < 0.2] = -1
    v, i = rerank_order(s, ids)
    wv, wi = _order_loops(s.tolist(), ids.tolist())
    assert v.tolist() == wv and i.tolist() == wi


def test_reranked_ranks_matches_loops():
    idx = torch.tensor([[4, 8, 2], [4, 8, 2], [4, 8, 2], [4, 8, 2], [6, -1, -1], [1, 5, 3]])
    order = torch.tensor([[2, 8, 4], [2, 4, 8], [8, 2, 4], [2, 8, 4], [6, -1, -1], [5, 3, 1]])
    # target at slot 0 moved last, at slot k-1 moved first, absent (stage-1 rank kept), moved to the
    # middle, a short list, and no target
    targets = torch.tensor([4, 2, 77, 8, 6, -1])
    first = torch.tensor([0, 2, 31, 1, 0, -1])
    got = reranked_ranks(first, idx, order, targets)
    want = []
    for f, irow, orow, t in zip(first.tolist(), idx.tolist(), order.tolist(), targets.tolist()):
        want.append(orow.index(t) if t >= 0 and t in irow else f)
    assert got.tolist() == want == [2, 0, 31, 1, 0, -1] and got.dtype == first.dtype
    one = reranked_ranks(torch.tensor([0, 9]), torch.tensor([[3], [3]]), torch.tensor([[3], [3]]), torch.tensor([3, 5]))
    assert one.tolist() == [0, 9]                                                    # k = 1 changes nothing


def test_xattn_mq_schema_and_fake():
    assert "xattn_mq" in torch_ops.OPS
    s = str(torch.ops.ste.xattn_mq.default._schema)
    assert s.startswith("ste::xattn_mq(Tensor q, Tensor qrow, Tensor k, Tensor v, Tensor? mask, SymInt C, SymInt nh)") \
        or s.startswith("ste::xattn_mq(Tensor q, Tensor qrow, Tensor k, Tensor v, Tensor? mask, int C, int nh)"), s
    assert s.endswith("-> Tensor")
    with FakeTensorMode():
        B, C, S, P = 3, 5, 49, 128
        kv = torch.empty(B * S, P, dtype=torch.bfloat16)
        out = torch.ops.ste.xattn_mq(torch.empty(7, P), torch.empty(B * C, dtype=torch.int32), kv, kv, None, C, 8)
        assert out.shape == (B * C, P) and out.dtype == torch.float32
        out = torch.ops.ste.xattn_mq(torch.empty(7, P), torch.empty(B * C, dtype=torch.int32), kv, kv,
                                     torch.empty(B * S, dtype=torch.int32), C, 8)
        assert out.shape == (B * C, P) and out.dtype == torch.float32


def test_xattn_argument_errors_return_status_without_launch():
    """Every contract violation of the two entry points is STE_ERR_SHAPE, returned before a launch
    (this box has no GPU: a launch would fail differently).  Pointers are never dereferenced."""
    from speech_transcript_embeddings_amd import _lib
    ERR_SHAPE = 1002
    mq, ga = _lib.fn("ste_xattn_mq_fwd"), _lib.fn("ste_xattn_gather_fwd")
    A = 1 << 20  # an aligned address

    def call_mq(B=2, C=4, S=50, P=128, nh=8, ldkv=256, k=A, v=A, out=A):
        return mq(A, A, k, v, ldkv, None, B, C, S, P, nh, 0.25, out, None)

    def call_ga(R=6, S=12, P=128, nh=8, ldkv=256, k=A, v=A, out=A):
        return ga(A, A, k, v, ldkv, A, None, R, S, P, nh, 0.25, out, None)

    for f in (call_mq, call_ga):
        assert f(P=100, nh=8) == ERR_SHAPE                # P % nh != 0
        assert f(P=96, nh=8, ldkv=192) == ERR_SHAPE       # dh = 12: dh % 8 != 0
        assert f(P=1024, nh=2, ldkv=2048) == ERR_SHAPE    # dh = 512 > 256
        assert f(P=2048, nh=8, ldkv=4096) == ERR_SHAPE    # P > 1024
        assert f(ldkv=260) == ERR_SHAPE                   # ldkv % 8 != 0
        assert f(S=0) == ERR_SHAPE
        for name in ("k", "v", "out"):                    # 16-byte alignment
            assert f(**{name: A + 8}) == ERR_SHAPE, name
    assert call_mq(C=0) == ERR_SHAPE
    assert call_mq(B=0) == ERR_SHAPE
    assert call_ga(R=0) == ERR_SHAPE
