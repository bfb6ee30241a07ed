"""Text -> clip reranking without a GPU: the pair plan of plan_clip_pairs against
brute-force loops, the composition of rerank_order / reranked_ranks into text -> audio ranks, the
ste::xattn_seg schema and fake implementation, the argument contract of ste_xattn_seg_fwd (which
returns before any launch) and the defaults that keep evaluate_retrieval as it was."""
import inspect

import pytest
import torch
from torch._subclasses.fake_tensor import FakeTensorMode

import speech_transcript_embeddings_amd as ste
from speech_transcript_embeddings_amd import torch_ops
from speech_transcript_embeddings_amd.retrieval import plan_clip_pairs, rerank_order, reranked_ranks

NEG = float("-inf")
# duplicate clips within and across rows, -1 slots, an all-empty row
IDX = [[7, 3, 7, 9], [3, -1, 11, 3], [-1, -1, -1, -1], [0, 9, -1, 2]]


def test_names_are_exported():
    for name in ("AudioStateStore", "plan_clip_pairs", "rerank_clips"):
        assert callable(getattr(ste, name))


def _check_plan(idx):
    """Every property of the plan, from loops over the candidate lists."""
    Q, k = idx.shape
    plan = plan_clip_pairs(idx)
    flat = idx.reshape(-1).tolist()
    live = [(v, j) for j, v in enumerate(flat) if v >= 0]
    want_order = [j for _, j in sorted(live)] + [j for j, v in enumerate(flat) if v < 0]   # stable by clip, -1 last
    unique = sorted({v for v in flat if v >= 0})
    assert plan["unique"].tolist() == unique and plan["unique"].dtype == idx.dtype
    assert plan["order"].tolist() == want_order
    R = Q * k
    pseg, qrow = plan["pseg"].tolist(), plan["qrow"].tolist()
    assert plan["pseg"].dtype == torch.int32 and plan["qrow"].dtype == torch.int32
    for j, slot in enumerate(want_order):
        v = flat[slot]
        assert pseg[j] == (unique.index(v) if v >= 0 else -1)
        assert qrow[j] == (slot // k if v >= 0 else -1)
    n_live = len(live)
    assert all(p >= 0 for p in pseg[:n_live]) and all(p < 0 for p in pseg[n_live:])
    assert pseg[:n_live] == sorted(pseg[:n_live])
    # the inverse permutation restores [Q, k]
    assert plan["inverse"].shape == idx.shape
    sorted_vals = torch.tensor([flat[s] for s in want_order], dtype=idx.dtype)
    assert torch.equal(sorted_vals[plan["inverse"]], idx)
    assert sorted(plan["inverse"].reshape(-1).tolist()) == list(range(R))
    # tiles: a partition of the live pairs, in order, one segment each, at most 16 pairs
    first, cnt = plan["tile_first"].tolist(), plan["tile_cnt"].tolist()
    assert plan["tile_first"].dtype == torch.int32 and plan["tile_cnt"].dtype == torch.int32 and len(first) == len(cnt)
    at = 0
    for f, c in zip(first, cnt):
        assert f == at and 1 <= c <= 16
        assert len(set(pseg[f:f + c])) == 1 and pseg[f] >= 0
        at += c
    assert at == n_live                                     # the -1 pairs belong to no tile
    per_clip = {v: flat.count(v) for v in unique}
    assert len(first) == sum((c + 15) // 16 for c in per_clip.values())
    return plan


@pytest.mark.parametrize("dtype", [torch.int32, torch.int64])
def test_plan_clip_pairs_matches_loops(dtype):
    _check_plan(torch.tensor(IDX, dtype=dtype))


def test_plan_clip_pairs_hub_clip_and_skew():
    """A clip retrieved by 40 queries gets 3 tiles (16, 16, 8); the clips retrieved once get one each."""
    g = torch.Generator().manual_seed(3)
    Q, k = 40, 5
    idx = torch.empty(Q, k, dtype=torch.int32)
    idx[:, 0] = 1000 + torch.randperm(Q, generator=g).to(torch.int32)   # distinct
    idx[:, 1] = 17                                                       # the hub, in every list
    idx[:, 2] = torch.randint(0, 6, (Q,), generator=g)
    idx[:, 3] = -1
    idx[:, 4] = torch.randint(-1, 3, (Q,), generator=g)
    idx = idx[:, torch.randperm(k, generator=g)]
    plan = _check_plan(idx)
    hub = plan["unique"].tolist().index(17)
    tiles = [(f, c) for f, c in zip(plan["tile_first"].tolist(), plan["tile_cnt"].tolist())
             if plan["pseg"][f].item() == hub]
    assert [c for _, c in tiles] == [16, 16, 8]
    # stable: the hub's pairs keep their query order
    f0 = tiles[0][0]
    assert plan["qrow"][f0:f0 + 40].tolist() == list(range(40))


def test_plan_clip_pairs_edges():
    plan = _check_plan(torch.full((3, 4), -1, dtype=torch.int32))      # nothing retrieved
    assert plan["unique"].numel() == 0 and plan["tile_first"].numel() == 0 and plan["tile_cnt"].numel() == 0
    assert plan["pseg"].tolist() == [-1] * 12 and plan["qrow"].tolist() == [-1] * 12
    plan = _check_plan(torch.tensor([[5]], dtype=torch.int32))          # Q = k = 1
    assert plan["tile_first"].tolist() == [0] and plan["tile_cnt"].tolist() == [1]
    _check_plan(torch.tensor([[4] * 16, [4] * 16], dtype=torch.int64))  # exactly two full tiles
    _check_plan(torch.tensor([[4] * 17], dtype=torch.int64))            # 16 + 1
    with pytest.raises(ValueError):
        plan_clip_pairs(torch.tensor([1, 2, 3]))


def test_scores_in_pair_order_come_back_through_the_inverse():
    """What Engine.score_clips does with the plan: a score computed per sorted pair lands in its slot."""
    idx = torch.tensor(IDX)
    plan = plan_clip_pairs(idx)
    k = idx.shape[1]
    fake = {(q, c): 10.0 * q + c for q in range(4) for c in range(k)}
    per_pair = torch.tensor([fake[(s // k, s % k)] for s in plan["order"].tolist()])
    got = per_pair.index_select(0, plan["inverse"].reshape(-1)).view(idx.shape)
    assert got.tolist() == [[10.0 * q + c for c in range(k)] for q in range(4)]


def test_rerank_order_and_reranked_ranks_compose_into_t2a_ranks():
    """Text query i's partner is clip i.  Stage 1 retrieved idx; fake fused scores reorder each list;
    the partner's rank is its reranked position when retrieved, else its stage-1 rank."""
    idx = torch.tensor([[2, 0, 5], [1, 4, -1], [0, 3, 4], [-1, -1, -1]], dtype=torch.int32)
    scores = torch.tensor([[0.1, 0.9, 0.5], [0.3, 0.7, 9.0], [0.2, 0.2, 0.1], [1.0, 2.0, 3.0]])
    first = torch.tensor([1, 0, 7, 5])           # clip 2 was not retrieved for query 2; query 3 got nothing
    vals, order = rerank_order(scores, idx)
    assert order.tolist() == [[0, 5, 2], [4, 1, -1], [0, 3, 4], [-1, -1, -1]]
    assert vals[1].tolist() == [pytest.approx(0.7), pytest.approx(0.3), NEG] and vals[3].tolist() == [NEG] * 3
    tgt = torch.arange(4, dtype=torch.int32)
    ranks = reranked_ranks(first, idx, order, tgt)
    assert ranks.tolist() == [0, 1, 7, 5]        # 0: moved up to first; 1: moved down; 2, 3: stage-1 rank kept


def test_evaluate_retrieval_defaults_keep_the_old_behaviour():
    sig = inspect.signature(ste.evaluate_retrieval)
    assert sig.parameters["rerank_t2a"].default is False
    assert sig.parameters["rerank_k"].default == 0
    sig = inspect.signature(ste.AudioStateStore.__init__)
    assert sig.parameters["reserve_frames"].default == 0 and sig.parameters["device"].default == "cuda"


def test_xattn_seg_schema_and_fake():
    assert "xattn_seg" in torch_ops.OPS
    s = str(torch.ops.ste.xattn_seg.default._schema).replace("SymInt", "int")
    assert s == ("ste::xattn_seg(Tensor q, Tensor qrow, Tensor pseg, Tensor k, Tensor v, Tensor seg_row, "
                 "Tensor seg_len, Tensor tile_first, Tensor tile_cnt, int nh) -> Tensor"), s
    with FakeTensorMode():
        i32 = lambda *n: torch.empty(*n, dtype=torch.int32)                       # noqa: E731
        out = torch.ops.ste.xattn_seg(torch.empty(5, 64), i32(12), i32(12), torch.empty(300, 64, dtype=torch.bfloat16),
                                      torch.empty(300, 64, dtype=torch.bfloat16), torch.empty(4, dtype=torch.int64),
                                      i32(4), i32(6), i32(6), 8)
        assert out.shape == (12, 64) and out.dtype == torch.float32


def test_xattn_seg_argument_errors_return_before_a_launch():
    """Every shape / alignment violation comes back as STE_ERR_SHAPE; the pointers are never read."""
    from speech_transcript_embeddings_amd import _lib
    f = _lib.fn("ste_xattn_seg_fwd")
    ERR_SHAPE = 1002
    A = 4096                                                   # a 16-B aligned address that is never dereferenced

    def call(k=A, v=A, ldkv=128, ntile=1, R=1, G=1, P=64, nh=8, out=A):
        return f(A, A, A, k, v, ldkv, A, A, A, A, ntile, R, G, P, nh, 0.35, out, None)

    assert call(P=80, nh=8) == ERR_SHAPE                       # dh = 10: not a multiple of 8
    assert call(P=64, nh=7) == ERR_SHAPE                       # P % nh != 0
    assert call(P=2048, nh=8, ldkv=4096) == ERR_SHAPE          # P > 1024
    assert call(P=1024, nh=2, ldkv=2048) == ERR_SHAPE          # dh = 512 > 256
    assert call(R=0) == ERR_SHAPE and call(G=0) == ERR_SHAPE and call(ntile=0) == ERR_SHAPE
    assert call(ldkv=60) == ERR_SHAPE and call(ldkv=132) == ERR_SHAPE    # ldkv < P; ldkv % 8 != 0
    assert call(out=A + 4) == ERR_SHAPE and call(k=A + 2) == ERR_SHAPE and call(v=A + 8) == ERR_SHAPE
