"""Corpus retrieval on the MI355X: ste_topk_sim / ste_topk_merge / EmbeddingIndex against a
float64 reference computed here (S on the CPU, ordered by np.lexsort((index, -S)); its logic is
checked against a brute-force loop in test_retrieval_cpu.py).

Exact cases: entries are integers in [-8, 8] and P <= 1024, so every product and partial sum is
at most 64 * 1024 = 65536 < 2^24 in magnitude: exact in fp32 in any order, and the entries are
exact in bf16.  Values, indices and ranks must then match the reference bit for bit.
The real-valued case uses b = 2 * P * 2^-24 (the fmaf-chain bound gamma_P times sum|a_k t_k| <= 1
for unit vectors, doubled); no measured tolerance enters."""
import numpy as np
import pytest
import torch

from retrieval_ref import lexsort_topk, ref_ranks, scores64

pytestmark = pytest.mark.gpu
DEV = "cuda"
KMAX = 128


def ints(rng, *shape):
    return rng.integers(-8, 9, size=shape).astype(np.float32)


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return t if dtype is None else t.to(dtype)


def check_exact(got, want_v, want_i, k, msg):
    v, i = got[0].cpu().numpy(), got[1].cpu().numpy()
    assert v.dtype == np.float32 and i.dtype == np.int32 and v.shape == i.shape == (want_v.shape[0], k), msg
    assert np.array_equal(i, want_i[:, :k]), msg
    assert np.array_equal(v.astype(np.float64), want_v[:, :k]), msg


@pytest.mark.parametrize("P", [4, 20, 66, 256])
def test_exact_sweep(P):
    """Every (Q, N, k, splits) of the grid at one P: N < k (the -inf / -1 tail), Q and N off the
    tile, P off the k-step (20, 66), N % splits != 0, empty slices (7 slices of 16 tiles), and
    more slices than tiles (clamped).  fp32 and bf16 storage agree bitwise; the rank of a random
    target (ties included, -1 = none) is its place in the reference order."""
    from speech_transcript_embeddings_amd import ops
    rng = np.random.default_rng(1000 + P)
    for N in (1, 5, 63, 64, 65, 1000):
        c = ints(rng, N, P)
        c32, c16 = dev(c), dev(c, torch.bfloat16)
        for Q in (1, 17, 33, 70):
            q = ints(rng, Q, P)
            S = scores64(q, c)
            base = int(rng.integers(0, 5000))
            want_v, want_i = lexsort_topk(S, KMAX, base)
            tgt = rng.integers(-1, N, size=Q)
            want_r = ref_ranks(S, tgt)
            qd = dev(q)
            td = dev(np.where(tgt >= 0, tgt + base, -1).astype(np.int32))
            for k in (1, 10, 128):
                for splits in (1, 2, 7):
                    msg = f"Q={Q} N={N} P={P} k={k} splits={splits}"
                    g32 = ops.topk_sim(qd, c32, k, index_base=base, target=td, splits=splits)
                    g16 = ops.topk_sim(qd, c16, k, index_base=base, target=td, splits=splits)
                    check_exact(g32, want_v, want_i, k, msg)
                    assert np.array_equal(g32[2].cpu().numpy(), want_r), msg
                    for a, b in zip(g32, g16):
                        assert torch.equal(a, b), msg + " (bf16 vs fp32 storage)"


def test_automatic_splits_and_no_target():
    from speech_transcript_embeddings_amd import ops
    rng = np.random.default_rng(7)
    q, c = ints(rng, 33, 66), ints(rng, 1000, 66)
    want_v, want_i = lexsort_topk(scores64(q, c), 10)
    got = ops.topk_sim(dev(q), dev(c), 10)
    assert len(got) == 2
    check_exact(got, want_v, want_i, 10, "auto splits")
    v, i = torch.ops.ste.topk_sim(dev(q), dev(c), 10)
    check_exact((v, i), want_v, want_i, 10, "torch op")


def test_widest_rows():
    """P = 1024, the widest row the kernel holds on chip (its largest LDS footprint), k = 128."""
    from speech_transcript_embeddings_amd import ops
    rng = np.random.default_rng(9)
    q, c = ints(rng, 33, 1024), ints(rng, 130, 1024)
    S = scores64(q, c)
    want_v, want_i = lexsort_topk(S, KMAX)
    tgt = rng.integers(-1, 130, size=33)
    for splits in (1, 2):
        for cd in (dev(c), dev(c, torch.bfloat16)):
            got = ops.topk_sim(dev(q), cd, 128, target=dev(tgt.astype(np.int32)), splits=splits)
            check_exact(got, want_v, want_i, 128, f"P=1024 splits={splits} {cd.dtype}")
            assert np.array_equal(got[2].cpu().numpy(), ref_ranks(S, tgt))


def test_ties_duplicated_rows():
    """Duplicates of the best row inside a tile, across a tile edge (63|64), a slice edge (2
    slices of 8 tiles: 511|512) and a chunk edge (chunks of 300, 212, 488 rows: 299|300): equal
    scores come back in index order, whatever tile, slice or chunk computed them."""
    from speech_transcript_embeddings_amd import EmbeddingIndex, ops
    rng = np.random.default_rng(11)
    N, P, k = 1000, 20, 10
    q, c = ints(rng, 17, P), ints(rng, N, P)
    dup = [3, 7, 63, 64, 299, 300, 511, 512]
    c[dup] = np.sign(q[0]) * 8               # the best possible row for query 0
    S = scores64(q, c)
    want_v, want_i = lexsort_topk(S, k)
    assert want_i[0, :8].tolist() == dup and len(set(want_v[0, :8])) == 1
    for splits in (1, 2, 7):
        check_exact(ops.topk_sim(dev(q), dev(c), k, splits=splits), want_v, want_i, k, f"splits={splits}")
    for dtype in (torch.float32, torch.bfloat16):
        ix = EmbeddingIndex(P, dtype, DEV)
        for lo, hi in ((0, 300), (300, 512), (512, 1000)):
            ix.add(dev(c[lo:hi]))
        check_exact(ix.search(dev(q), k, splits=2), want_v, want_i, k, f"chunks {dtype}")
        assert np.array_equal(ix.ranks(dev(q), torch.tensor(dup + [0] * 9)).cpu().numpy(),
                              ref_ranks(S, np.array(dup + [0] * 9)))


@pytest.mark.parametrize("splits", [1, 2, 7])
def test_identical_rows(splits):
    from speech_transcript_embeddings_amd import ops
    rng = np.random.default_rng(13)
    N, P, base = 200, 66, 1000
    q = ints(rng, 33, P)
    c = np.repeat(ints(rng, 1, P), N, axis=0)
    for k in (1, 10, 128):
        v, i = ops.topk_sim(dev(q), dev(c), k, index_base=base, splits=splits)
        assert np.array_equal(i.cpu().numpy(), np.tile(base + np.arange(k, dtype=np.int32), (33, 1)))
        assert np.array_equal(v.cpu().numpy().astype(np.float64), np.repeat(scores64(q, c[:1]), k, axis=1))


@pytest.mark.parametrize("order", ["ascending", "descending"])
def test_adversarial_orders(order):
    """Query 0's scores are j - 496 for corpus row j (strictly ascending: every row enters the
    list) or the reverse (nothing enters after the first k)."""
    from speech_transcript_embeddings_amd import ops
    rng = np.random.default_rng(17)
    N, P = 1000, 20
    q = ints(rng, 17, P)
    q[0] = [8] * 16 + [1, 0, 0, 0]
    c = np.zeros((N, P), dtype=np.float32)
    for j in range(N):
        t, b = j // 8 - 62, j % 8
        c[j, :16] = t // 16 + (np.arange(16) < t % 16)
        c[j, 16] = b
    assert np.abs(c).max() <= 8 and np.array_equal(scores64(q[:1], c)[0], np.arange(N) - 496.0)
    if order == "descending":
        c = c[::-1].copy()
    S = scores64(q, c)
    want_v, want_i = lexsort_topk(S, KMAX)
    for k in (10, 128):
        for splits in (1, 2):
            got = ops.topk_sim(dev(q), dev(c), k, splits=splits)
            check_exact(got, want_v, want_i, k, f"{order} k={k} splits={splits}")
    top = np.arange(N - 1, N - 11, -1) if order == "ascending" else np.arange(10)
    assert want_i[0, :10].tolist() == top.tolist()


def test_ranks_special_targets():
    """Target = the top-1 index gives rank 0, -1 gives -1, and a target in another chunk than the
    best row (its score then travels as tscore) keeps its place in the reference order."""
    from speech_transcript_embeddings_amd import EmbeddingIndex, ops
    rng = np.random.default_rng(19)
    Q, N, P = 33, 1000, 66
    q, c = ints(rng, Q, P), ints(rng, N, P)
    S = scores64(q, c)
    _, top = lexsort_topk(S, 1)
    tgt = top[:, 0].copy()
    tgt[::5] = -1
    for splits in (1, 2, 7):
        r = ops.topk_sim(dev(q), dev(c), 10, target=dev(tgt.astype(np.int32)), splits=splits)[2].cpu().numpy()
        assert np.array_equal(r, np.where(tgt >= 0, 0, -1))
    ix = EmbeddingIndex(P, device=DEV)
    for lo, hi in ((0, 130), (130, 131), (131, 1000)):
        ix.add(dev(c[lo:hi]))
    assert len(ix) == N
    far = np.where(top[:, 0] < 131, 131 + (top[:, 0] * 7) % 869, top[:, 0] % 130)   # never the best row's chunk
    chunk_of = lambda i: np.searchsorted([130, 131], i, side="right")               # noqa: E731
    assert np.all(chunk_of(far) != chunk_of(top[:, 0]))
    assert np.array_equal(ix.ranks(dev(q), torch.from_numpy(far)).cpu().numpy(), ref_ranks(S, far))
    # the C ABI's tscore path directly: chunk 2 scans with the score computed on chunk 0
    t32 = dev(far.astype(np.int32))
    ts = torch.zeros(Q, device=DEV)
    ops.topk_target_score(dev(q), dev(c[:130]), t32, ts, index_base=0)
    ops.topk_target_score(dev(q), dev(c[131:]), t32, ts, index_base=131)
    assert np.array_equal(ts.cpu().numpy().astype(np.float64), S[np.arange(Q), far])
    part = ops.topk_sim(dev(q), dev(c[131:]), 1, index_base=131, target=t32, tscore=ts)[2].cpu().numpy()
    j = np.arange(131, N)
    want = [int(np.sum((S[r, 131:] > S[r, far[r]]) | ((S[r, 131:] == S[r, far[r]]) & (j < far[r])))) for r in range(Q)]
    assert part.tolist() == want


def test_index_chunks_equal_one_chunk_and_merge_sorts():
    from speech_transcript_embeddings_amd import EmbeddingIndex, ops
    rng = np.random.default_rng(23)
    Q, N, P, k = 70, 1000, 256, 10
    q, c = ints(rng, Q, P), ints(rng, N, P)
    want_v, want_i = lexsort_topk(scores64(q, c), KMAX)
    for dtype in (torch.float32, torch.bfloat16):
        one, three = EmbeddingIndex(P, dtype, DEV), EmbeddingIndex(P, dtype, DEV)
        one.add(dev(c))
        for lo, hi in ((0, 1), (1, 64), (64, 1000)):
            three.add(dev(c[lo:hi]))
        assert len(one) == len(three) == N
        for kk in (1, k, 128):
            a, b = one.search(dev(q), kk), three.search(dev(q), kk)
            check_exact(a, want_v, want_i, kk, f"one chunk {dtype}")
            assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    # topk_merge on shuffled candidates (ties and empty entries included) = sorting them
    L, C = 5, 5 * k
    vals = rng.integers(-3, 4, size=(Q, C)).astype(np.float32)
    idx = np.stack([rng.permutation(4 * C)[:C] for _ in range(Q)]).astype(np.int32)
    vals[:, -7:], idx[:, -7:] = -np.inf, -1
    perm = np.stack([rng.permutation(C) for _ in range(Q)])
    vals, idx = np.take_along_axis(vals, perm, 1), np.take_along_axis(idx, perm, 1)
    counts = rng.integers(0, 50, size=(Q, L)).astype(np.int32)
    counts[3, 2] = -1
    ov, oi, orank = ops.topk_merge(dev(vals), dev(idx), k, counts=dev(counts))
    ov_h, oi_h = ov.cpu().numpy(), oi.cpu().numpy()
    for r in range(Q):
        key_i = np.where(idx[r] < 0, np.iinfo(np.int32).max, idx[r])
        order = np.lexsort((key_i, -vals[r].astype(np.float64)))[:k]
        assert np.array_equal(ov_h[r], vals[r, order]) and np.array_equal(oi_h[r], idx[r, order])
    assert np.array_equal(orank.cpu().numpy(), np.where((counts < 0).any(1), -1, counts.sum(1)))
    # fewer candidates than k: the (-inf, -1) tail
    ov, oi = ops.topk_merge(dev(vals[:, :4]), dev(idx[:, :4]), k)
    assert torch.isneginf(ov[:, 4:]).all() and (oi[:, 4:] == -1).all()


def test_real_valued_bound():
    from speech_transcript_embeddings_amd import ops
    rng = np.random.default_rng(29)
    Q, N, P, k = 33, 1000, 256, 10
    q = rng.standard_normal((Q, P))
    c = rng.standard_normal((N, P))
    q = (q / np.linalg.norm(q, axis=1, keepdims=True)).astype(np.float32)
    c = (c / np.linalg.norm(c, axis=1, keepdims=True)).astype(np.float32)
    S = scores64(q, c)                      # float64 scores of the fp32 rows the kernel reads
    b = 2 * P * 2.0 ** -24
    for splits in (0, 1, 7):
        v, i = (t.cpu().numpy() for t in ops.topk_sim(dev(q), dev(c), k, splits=splits))
        v = v.astype(np.float64)
        assert np.all(v[:, :-1] >= v[:, 1:])
        for r in range(Q):
            assert len(set(i[r].tolist())) == k and i[r].min() >= 0 and i[r].max() < N
            assert np.all(np.abs(v[r] - S[r, i[r]]) <= b)
            rest = np.delete(S[r], i[r])
            assert rest.max() <= v[r, -1] + 2 * b


def test_search_memory():
    """search() never holds the Q x N matrix: its peak is the outputs, the planned workspace and
    allocator slack, well under an eighth of Q * N * 4 bytes."""
    from speech_transcript_embeddings_amd import EmbeddingIndex, ops
    Q, N, P, k = 256, 65536, 64, 10
    g = torch.Generator(device="cpu").manual_seed(31)
    ix = EmbeddingIndex(P, device=DEV)
    ix.add(torch.randint(-8, 9, (N, P), generator=g).float())
    q = torch.randint(-8, 9, (Q, P), generator=g).float().to(DEV)
    _, ws = ops.topk_sim_plan(Q, N, P, k)
    budget = Q * k * 8 + ws + (1 << 20)
    assert budget < Q * N * 4 // 8
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    v, i = ix.search(q, k)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    print(f"search peak {peak} B, budget {budget} B, matrix {Q * N * 4} B")
    assert peak <= budget
    # and the result is right: query r against its own copy planted in the corpus
    ix2 = EmbeddingIndex(P, device=DEV)
    rows = ix.chunks[0][1].clone()
    rows[1000:1000 + Q] = 8 * torch.sign(q)      # 8 * sum|q_r|: more than any other row can score
    ix2.add(rows)
    assert torch.equal(ix2.search(q, 1)[1][:, 0].cpu(), torch.arange(1000, 1000 + Q, dtype=torch.int32))


def test_end_to_end_embeddings_and_evaluate_retrieval():
    from test_model_gpu import batch_of, load, mini_model
    from speech_transcript_embeddings_amd import embed_audio, embed_texts, evaluate_retrieval, ops, retrieval_metrics
    meta, z = load("noalign")
    model = mini_model(meta)
    model.eval()
    b1 = batch_of(z)
    # second batch: the corrupted transcripts as clean ones, the clips in reverse order
    b2 = dict(b1, input_ids_pos=b1["input_ids_neg"], attention_mask_pos=b1["attention_mask_neg"],
              input_values=b1["input_values"].flip(0).contiguous(),
              attention_mask_audio=b1["attention_mask_audio"].flip(0).contiguous())
    T, A = [], []
    for b in (b1, b2):
        t, a = embed_texts(model, b["input_ids_pos"], b["attention_mask_pos"]), embed_audio(
            model, b["input_values"], b["attention_mask_audio"])
        with torch.no_grad():
            te = model.encode_text(b["input_ids_pos"], b["attention_mask_pos"])[0]
            ae = model.encode_audio(b["input_values"], b["attention_mask_audio"])[0]
        for got, raw in ((t, te), (a, ae)):
            assert not got.requires_grad and got.dtype == torch.float32
            want = torch.nn.functional.normalize(raw.double(), p=2, dim=1)
            # fp32 sum of P squares (relative error <= P * 2^-24, halved by the root), then the root,
            # the reciprocal / division and the product round once each; |components| <= 1
            assert (got.double() - want).abs().max().item() <= (raw.shape[1] / 2 + 4) * 2.0 ** -24
        T.append(t)
        A.append(a)
    T, A = torch.cat(T), torch.cat(A)
    n = T.shape[0]
    S = torch.empty(n, n, device=DEV)
    ops.similarity(A, T, S)
    a2t = ref_ranks(S.cpu().numpy().astype(np.float64), np.arange(n))
    ops.similarity(T, A, S)
    t2a = ref_ranks(S.cpu().numpy().astype(np.float64), np.arange(n))
    cpu = lambda b: {k: v.cpu() for k, v in b.items()}                                 # noqa: E731
    out = evaluate_retrieval(model, [cpu(b1), None, cpu(b2)], DEV, ks=(1, 2), return_ranks=True)
    assert np.array_equal(out["a2t_ranks"].cpu().numpy(), a2t)
    assert np.array_equal(out["t2a_ranks"].cpu().numpy(), t2a)
    assert out["a2t"] == retrieval_metrics(torch.from_numpy(a2t), ks=(1, 2)) and out["a2t"]["n"] == n
    assert out["t2a"] == retrieval_metrics(torch.from_numpy(t2a), ks=(1, 2))
    assert set(evaluate_retrieval(model, [cpu(b1)], DEV)) == {"a2t", "t2a"}
