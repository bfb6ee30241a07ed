"""Corpus retrieval on the HIP path: search the shared embedding space.

The reference exposes per-item embeddings (processor.py:128-146, get_text_embedding /
get_audio_embedding: encode_* projection, L2-normalised, no cross-modal fusion: the fused
embeddings depend on the pair, so they cannot be indexed) and compares them pair by pair.  This
module indexes them and answers the question a trained checkpoint is asked first: for this clip,
where does its transcript rank among all transcripts of the split, and the reverse.

    embed_texts(model, input_ids, attention_mask)        -> [B, P] unit rows
    embed_audio(model, input_values, attention_mask_audio) -> [B, P] unit rows
    EmbeddingIndex(dim, dtype, device): add(emb), len(), search(queries, k), ranks(queries, targets)
    retrieval_metrics(ranks, ks)                         -> recall@k, mrr, median_rank, n
    evaluate_retrieval(model, data_loader, device, ks)   -> {"a2t": metrics, "t2a": metrics}

Scores and selection run in ste_topk_sim (csrc/retrieval.hip): the queries x corpus score matrix
is never written.  The order is total (value descending, index ascending) and a row's score is
bit-identical wherever it is computed, so results do not depend on how the corpus was chunked.
"""
from __future__ import annotations

import torch

from . import ops

F32, BF16, I32 = torch.float32, torch.bfloat16, torch.int32


def _unit_rows(x: torch.Tensor) -> torch.Tensor:
    x = x.float().contiguous()
    y = torch.empty_like(x)
    ops.l2norm_fwd(x, y, torch.empty(x.shape[0], device=x.device, dtype=F32))
    return y


@torch.no_grad()
def embed_texts(model, input_ids, attention_mask=None) -> torch.Tensor:
    """processor.py:128-136: F.normalize(model.encode_text(...)[0]), forward-only."""
    return _unit_rows(model.encode_text(input_ids, attention_mask)[0])


@torch.no_grad()
def embed_audio(model, input_values, attention_mask_audio=None) -> torch.Tensor:
    """processor.py:138-146: F.normalize(model.encode_audio(...)[0]), forward-only."""
    return _unit_rows(model.encode_audio(input_values, attention_mask_audio)[0])


class EmbeddingIndex:
    """Rows of one modality's embeddings, appended in chunks; a chunk's rows keep the global
    indices base .. base + len(chunk) - 1.  dtype float32 stores the rows as given, bfloat16
    rounds them to bf16 (half the bytes streamed per search; scores are then those of the
    rounded rows, still computed in fp32)."""

    def __init__(self, dim: int, dtype: torch.dtype = F32, device="cuda"):
        if dtype not in (F32, BF16):
            raise TypeError(f"EmbeddingIndex stores float32 or bfloat16 rows, got {dtype}")
        self.dim, self.dtype, self.device = int(dim), dtype, torch.device(device)
        self.chunks: list[tuple[int, torch.Tensor]] = []   # (base index, rows [n, dim])
        self._n = 0

    def __len__(self) -> int:
        return self._n

    def add(self, emb: torch.Tensor) -> None:
        if emb.dim() != 2 or emb.shape[1] != self.dim:
            raise ValueError(f"expected rows of width {self.dim}, got {tuple(emb.shape)}")
        if emb.shape[0] == 0:
            return
        if self._n + emb.shape[0] > 2**31 - 1:
            raise ValueError("an EmbeddingIndex holds fewer than 2^31 rows")
        rows = emb.detach().to(self.device)
        if self.dtype == BF16 and rows.dtype != BF16:
            rows = ops.cast_bf16(rows.float().contiguous(), torch.empty(rows.shape, device=self.device, dtype=BF16))
        rows = rows.to(self.dtype).contiguous()
        if rows.data_ptr() == emb.data_ptr():
            rows = rows.clone()   # the index owns its rows
        self.chunks.append((self._n, rows))
        self._n += rows.shape[0]

    def _queries(self, queries: torch.Tensor) -> torch.Tensor:
        if queries.dim() != 2 or queries.shape[1] != self.dim:
            raise ValueError(f"expected queries of width {self.dim}, got {tuple(queries.shape)}")
        if not self.chunks:
            raise ValueError("the index is empty")
        return queries.detach().to(self.device, F32).contiguous()

    def search(self, queries: torch.Tensor, k: int, *, splits: int = 0):
        """(values fp32 [Q, k], indices int32 [Q, k]) of the k best rows per query; with fewer
        than k rows in the index the tail is (-inf, -1)."""
        q = self._queries(queries)
        parts = [ops.topk_sim(q, rows, k, index_base=base, splits=splits) for base, rows in self.chunks]
        if len(parts) == 1:
            return parts[0]
        return ops.topk_merge(torch.cat([p[0] for p in parts], 1), torch.cat([p[1] for p in parts], 1), k)

    def ranks(self, queries: torch.Tensor, targets: torch.Tensor, *, splits: int = 0) -> torch.Tensor:
        """0-based rank int64 [Q] of row targets[i] for query i: the number of rows that order
        before it (value descending, index ascending); -1 where targets[i] < 0.  Targets are
        indices into this index."""
        q = self._queries(queries)
        tgt = targets.detach().to(self.device, I32).contiguous()
        if tgt.shape != (q.shape[0],):
            raise ValueError(f"expected {q.shape[0]} targets, got {tuple(tgt.shape)}")
        tscore = torch.zeros(q.shape[0], device=self.device, dtype=F32)
        for base, rows in self.chunks:     # each target's score, from the chunk that holds it
            ops.topk_target_score(q, rows, tgt, tscore, index_base=base)
        counts = [ops.topk_sim(q, rows, 1, index_base=base, target=tgt, tscore=tscore, splits=splits)[2]
                  for base, rows in self.chunks]
        total = torch.stack(counts, 1).to(torch.int64).sum(1)   # integer counts: any order gives the same sum
        return torch.where(tgt >= 0, total, torch.full_like(total, -1))


def retrieval_metrics(ranks: torch.Tensor, ks=(1, 5, 10)) -> dict:
    """recall@k = mean(rank < k), mrr = mean(1 / (rank + 1)), median_rank (1-based) and n over the
    0-based ranks >= 0 (negative entries mean "no target" and are ignored).  CPU or GPU tensor;
    one host transfer."""
    r = torch.as_tensor(ranks).reshape(-1)
    r = r[r >= 0].to(torch.float64)
    n = int(r.numel())
    out = {f"recall@{k}": 0.0 for k in ks}
    out.update(mrr=0.0, median_rank=0.0, n=n)
    if n == 0:
        return out
    stats = torch.stack([(r < k).to(torch.float64).mean() for k in ks]
                        + [(1.0 / (r + 1.0)).mean(), torch.quantile(r, 0.5) + 1.0]).cpu().tolist()
    for k, v in zip(ks, stats):
        out[f"recall@{k}"] = v
    out["mrr"], out["median_rank"] = stats[-2], stats[-1]
    return out


@torch.no_grad()
def evaluate_retrieval(model, data_loader, device, ks=(1, 5, 10), index_dtype: torch.dtype = F32,
                       return_ranks: bool = False) -> dict:
    """One pass over a loader of the reference's batch dicts (custom_collate_fn's keys): embeds the
    clean transcripts and the audio, indexes both and ranks pair i's partner for query i in both
    directions.  Returns {"a2t": retrieval_metrics, "t2a": retrieval_metrics} (audio -> text,
    text -> audio), plus the rank tensors under "a2t_ranks" / "t2a_ranks" on request.  None
    batches are skipped, as evaluate() does; everything stays on the device until the metrics are
    read."""
    model.eval()
    texts, audios = [], []
    text_index = audio_index = None
    for batch in data_loader:
        if batch is None:
            continue
        b = {k: v.to(device, non_blocking=True) if isinstance(v, torch.Tensor) else v for k, v in batch.items()}
        t = embed_texts(model, b["input_ids_pos"], b["attention_mask_pos"])
        a = embed_audio(model, b["input_values"], b.get("attention_mask_audio"))
        if text_index is None:
            text_index = EmbeddingIndex(t.shape[1], index_dtype, t.device)
            audio_index = EmbeddingIndex(a.shape[1], index_dtype, a.device)
        text_index.add(t)
        audio_index.add(a)
        texts.append(t)
        audios.append(a)
    if text_index is None:
        a2t = t2a = torch.empty(0, dtype=torch.int64)
    else:
        pair = torch.arange(len(text_index), device=text_index.device, dtype=I32)
        a2t = text_index.ranks(torch.cat(audios), pair)
        t2a = audio_index.ranks(torch.cat(texts), pair)
    out = {"a2t": retrieval_metrics(a2t, ks), "t2a": retrieval_metrics(t2a, ks)}
    if return_ranks:
        out.update(a2t_ranks=a2t, t2a_ranks=t2a)
    return out
