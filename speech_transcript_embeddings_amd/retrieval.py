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

Stage 2 rescores a clip's k retrieved transcripts with the fused pair score the model is
trained on (model.score_candidates: one audio pass per clip, one text pass per distinct candidate):

    plan_candidates(idx)                          -> (unique ids [U], slots [Q, k] into them)
    rerank_order(scores, idx)                     -> (values, indices), score descending
    reranked_ranks(first_ranks, idx, order, tgt)  -> the target's rank after reranking
    rerank(model, input_values, attention_mask_audio, text_ids, text_mask, idx) -> (values, indices)
    evaluate_retrieval(..., rerank_k=k)           -> also "a2t_rerank"

The other direction, a typed phrase against the corpus of clips, needs the audio states
of every clip; they are computed once when the corpus is indexed and attended over in place:

    AudioStateStore(model): add(input_values, mask), len(), frames, nbytes, search(text_emb, k)
    AudioStateStore(model, kv_dtype="mx8"): the K/V rows as MX-fp8 at 0.516 of the bytes;
        kv_rows(n), kv_bytes_per_frame(dim, kv_dtype)
    plan_clip_pairs(idx)                          -> the (query, clip) pairs grouped by clip, in tiles
    rerank_clips(model, input_ids, attention_mask, store, idx) -> (values, indices)
    evaluate_retrieval(..., rerank_k=k, rerank_t2a=True) -> also "t2a_rerank"
    AudioStateStore(model, align_rows=True): also the alignment head's K|V rows;
        align_kv_rows(n), align_bytes_per_frame(dim)
    search_clips(model, store, input_ids, attention_mask, k) -> (values, indices, where in each hit)

Recordings of minutes to hours are encoded chunk by chunk, stored once and indexed as
overlapping windows that are views of the stored rows:

    plan_recording(frames, window, hop, chunk, context) -> the chunks and the windows
    AudioStateStore.add_recording(features [F, 160]) -> recording id; recording_of, offset_of, recordings
    best_per_recording(values, idx, recording_of, k) -> each recording's best window, in order
    search_recordings(model, store, input_ids, attention_mask, k) -> (values, recordings, windows, where)

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


# ------------------------------------------------------------------- stage 2: rerank
def plan_candidates(idx: torch.Tensor):
    """Candidate lists idx [Q, k] (corpus ids, -1 = empty) -> (unique ids [U] ascending, slots [Q, k]
    with idx == unique[slots] and -1 kept as -1), so that each distinct candidate is encoded once.
    Pure torch, any device."""
    idx = torch.as_tensor(idx)
    valid = idx >= 0
    unique = torch.unique(idx[valid])
    slots = torch.searchsorted(unique, idx.clamp(min=0).contiguous()).to(idx.dtype)
    return unique, torch.where(valid, slots, torch.full_like(slots, -1))


def rerank_order(scores: torch.Tensor, idx: torch.Tensor):
    """Reorder candidate lists idx [Q, k] by scores [Q, k]: score descending, ties by stage-1
    position ascending (a total order), empty slots (idx < 0) last as (-inf, -1).  Returns
    (values [Q, k], indices [Q, k]) like EmbeddingIndex.search.  Pure torch, any device."""
    idx = torch.as_tensor(idx)
    empty = idx < 0
    s = torch.where(empty, torch.full_like(scores, float("-inf")), scores)
    order = torch.sort(s, dim=1, descending=True, stable=True)[1]
    # empties after every real candidate, whatever its score: a second stable sort on the flag
    order = order.gather(1, torch.sort(empty.gather(1, order).to(torch.int8), dim=1, stable=True)[1])
    return s.gather(1, order), torch.where(empty, torch.full_like(idx, -1), idx).gather(1, order)


def reranked_ranks(first_ranks: torch.Tensor, idx: torch.Tensor, order_indices: torch.Tensor,
                   targets: torch.Tensor) -> torch.Tensor:
    """The target's 0-based rank after reranking the k first candidates idx [Q, k] into
    order_indices [Q, k]: its position in the reranked list if it is among them, else its stage-1
    rank first_ranks [Q] (reranking permutes the first k places only, so recall@m for m >= k
    cannot change).  targets < 0 (no target) keep first_ranks.  Pure torch, any device."""
    tgt = torch.as_tensor(targets).to(order_indices.dtype).reshape(-1, 1)
    among = ((torch.as_tensor(idx) == tgt) & (tgt >= 0)).any(1)
    pos = ((order_indices == tgt) & (tgt >= 0)).to(torch.int8).argmax(1)
    return torch.where(among, pos.to(first_ranks.dtype), first_ranks)


@torch.no_grad()
def rerank(model, input_values, attention_mask_audio, text_ids, text_mask, idx, *, audio_encoded=None):
    """Rerank each clip's retrieved transcripts idx [B, k] (rows of the token store text_ids /
    text_mask [N, L], as returned by a text index's search) with the fused pair score:
    plan_candidates -> gather the distinct rows -> model.score_candidates -> rerank_order.
    Returns (values fp32 [B, k], indices [B, k]).  audio_encoded: see score_candidates."""
    unique, slots = plan_candidates(idx)
    if unique.numel() == 0:
        return rerank_order(torch.zeros(idx.shape, device=idx.device, dtype=F32), idx)
    rows = unique.to(text_ids.device, torch.int64)
    scores = model.score_candidates(input_values, attention_mask_audio, text_ids.index_select(0, rows),
                                    text_mask.index_select(0, rows), slots, audio_encoded=audio_encoded)
    return rerank_order(scores, idx.to(scores.device))


# ------------------------------------------------- stage 2, text -> clips
def plan_clip_pairs(idx: torch.Tensor) -> dict:
    """Candidate lists idx [Q, k] of clip ids (-1 = empty) -> the (query, clip) pairs grouped for
    ste_xattn_seg_fwd.  The R = Q·k pairs are sorted by clip with a stable sort, so pairs of one clip
    keep their (query, column) order and the empty ones come last; the distinct clips become the
    segments through plan_candidates.  Returns a dict of
        unique      [G] the distinct clip ids, ascending (dtype of idx)
        order       int64 [R]: sorted pair j is flat slot order[j] = query·k + column
        inverse     int64 [Q, k]: slot (q, c) is sorted pair inverse[q, c] (sorted[inverse] restores [Q, k])
        qrow        int32 [R]: the query of sorted pair j, -1 for an empty pair
        pseg        int32 [R]: its segment (index into unique), non-decreasing, -1 for an empty pair
        tile_first, tile_cnt  int32 [tiles]: tile t holds the sorted pairs tile_first[t] ..
                    tile_first[t] + tile_cnt[t] - 1, all of one segment and at most 16; a clip
                    retrieved by c queries gets ceil(c / 16) tiles and the empty pairs get none.
    Pure torch, any device."""
    idx = torch.as_tensor(idx)
    if idx.dim() != 2:
        raise ValueError(f"candidate lists must be [Q, k], got {tuple(idx.shape)}")
    k = max(int(idx.shape[1]), 1)
    dev = idx.device
    unique, slots = plan_candidates(idx)
    G = unique.numel()
    flat = slots.reshape(-1).to(torch.int64)
    order = torch.sort(torch.where(flat >= 0, flat, torch.full_like(flat, G)), stable=True)[1]
    pseg = flat[order]
    R = order.numel()
    inverse = torch.empty_like(order)
    inverse[order] = torch.arange(R, device=dev)
    qrow = torch.where(pseg >= 0, order // k, torch.full_like(order, -1))
    counts = torch.bincount(flat[flat >= 0], minlength=G)            # pairs per segment
    ntile = (counts + 15) // 16
    seg = torch.repeat_interleave(torch.arange(G, device=dev), ntile)                 # segment of each tile
    within = torch.arange(seg.numel(), device=dev) - (torch.cumsum(ntile, 0) - ntile)[seg]
    tile_first = (torch.cumsum(counts, 0) - counts)[seg] + 16 * within
    tile_cnt = torch.clamp(counts[seg] - 16 * within, max=16)
    return dict(unique=unique, order=order, inverse=inverse.view(idx.shape), qrow=qrow.to(I32), pseg=pseg.to(I32),
                tile_first=tile_first.to(I32), tile_cnt=tile_cnt.to(I32))


KV_DTYPES = ("bf16", "mx8")
ALIGN_MAX_FRAMES = 2048   # the T limit of ste_align_matrix_seg_fwd and ste_align_decode
POOL_MAX_FRAMES = 8192    # the longest segment ste_attn_pool_seg_fwd pools (and ste_attn_pool_fwd's L limit)


# ------------------------------------------------- long recordings
def plan_recording(frames: int, window_frames: int, hop_frames: int, chunk_frames: int, context_frames: int, *,
                   max_window: int = POOL_MAX_FRAMES) -> dict:
    """How a recording of F = frames encoder frames is encoded and indexed (AudioStateStore.add_recording).

    Chunks: the kept ranges [c·chunk, min((c+1)·chunk, F)) partition [0, F); the encoder input of chunk c
    is its kept range widened by context_frames on both sides and clipped to [0, F), so a kept frame
    sees at least that much context unless the recording ends sooner.

    Windows: starts 0, hop, 2·hop, ...; one window if F <= window, else ceil((F - window) / hop) + 1;
    window i has min(window, F - start) frames (only the last can be shorter, and it still has more than
    window - hop).  Consequence: every span of at most window - hop + 1 frames lies wholly inside some
    window (the one starting at the last multiple of hop at or before the span, or the last window), which
    is what lets a free-endpoint locate find a phrase that straddles a window boundary.

    Returns a dict of Python ints and lists: frames; keep and input, the (first, last + 1) ranges of each
    chunk; window_start and window_len.  ValueError unless 1 <= hop <= window <= max_window (8192, the
    pooling kernel's segment limit; an align_rows store passes ALIGN_MAX_FRAMES), chunk >= 1,
    context >= 0 and F >= 1.  Pure Python."""
    F, W, hop, chunk, ctx = (int(v) for v in (frames, window_frames, hop_frames, chunk_frames, context_frames))
    if F < 1:
        raise ValueError(f"a recording has at least one frame, got {F}")
    if not 1 <= hop <= W <= int(max_window):
        raise ValueError(f"need 1 <= hop_frames <= window_frames <= {int(max_window)}, got hop_frames={hop}, "
                         f"window_frames={W}")
    if chunk < 1 or ctx < 0:
        raise ValueError(f"need chunk_frames >= 1 and context_frames >= 0, got {chunk} and {ctx}")
    keep = [(a, min(a + chunk, F)) for a in range(0, F, chunk)]
    inputs = [(max(a - ctx, 0), min(b + ctx, F)) for a, b in keep]
    nwin = 1 if F <= W else -(-(F - W) // hop) + 1
    starts = [i * hop for i in range(nwin)]
    return dict(frames=F, keep=keep, input=inputs, window_start=starts, window_len=[min(W, F - s) for s in starts])


def best_per_recording(values: torch.Tensor, idx: torch.Tensor, recording_of: torch.Tensor, k: int):
    """Window lists -> recording lists.  values / idx [Q, m]: each query's windows best-first, as
    store.search or rerank_order return them (-1 = empty slot); recording_of int [N]: the recording of
    each window.  Keeps, per row and in order, the first (best) window of each recording ->
    (values fp32 [Q, k], recordings [Q, k], windows [Q, k]), padded with (-inf, -1, -1); k may exceed m or
    the number of distinct recordings.  Pure torch, any device, no host sync."""
    idx = torch.as_tensor(idx)
    if idx.dim() != 2 or values.shape != idx.shape:
        raise ValueError(f"values and idx must both be [Q, m], got {tuple(values.shape)} and {tuple(idx.shape)}")
    k = int(k)
    if k < 1:
        raise ValueError(f"k must be at least 1, got {k}")
    Q, m = idx.shape
    dev = idx.device
    live = idx >= 0
    rec = recording_of.to(dev).to(idx.dtype)
    rec = (torch.where(live, rec[idx.clamp(min=0).long()], torch.full_like(idx, -1)) if rec.numel()
           else torch.full_like(idx, -1))
    live = live & (rec >= 0)
    earlier = torch.ones(m, m, dtype=torch.bool, device=dev).tril(-1)             # [j, j'] with j' < j
    dup = ((rec.unsqueeze(2) == rec.unsqueeze(1)) & earlier & live.unsqueeze(1)).any(2)
    keep = live & ~dup
    order = torch.sort((~keep).to(torch.int8), dim=1, stable=True)[1]             # the kept slots first, in order
    keep = keep.gather(1, order)
    vals = torch.where(keep, values.gather(1, order).float(), torch.full((), float("-inf"), device=dev))
    recs = torch.where(keep, rec.gather(1, order), torch.full_like(idx, -1))
    wins = torch.where(keep, idx.gather(1, order), torch.full_like(idx, -1))
    if m < k:
        pad = (0, k - m)
        return (torch.nn.functional.pad(vals, pad, value=float("-inf")), torch.nn.functional.pad(recs, pad, value=-1),
                torch.nn.functional.pad(wins, pad, value=-1))
    return vals[:, :k].contiguous(), recs[:, :k].contiguous(), wins[:, :k].contiguous()


class RowBank:
    """K|V rows of width 2·dim in one growable buffer, held as bf16 or as MX-fp8:
      "bf16"  data bf16 [capacity, 2·dim], scales None: 4·dim bytes per row;
      "mx8"   data uint8 [capacity, 2·dim] of OCP e4m3 bytes + scales uint8 [capacity, 2·dim/32] of E8M0
              block scales (one per 32 columns), ops.mx8_quant of each bf16 row as it is written:
              2·dim + dim/16 bytes per row.  Needs dim % 64 == 0.
    arg is the caller's name for dtype, for the ValueErrors.  held=False is the bank of a store that keeps
    no such rows: empty, and dim is not checked.  The owner counts the rows in use."""

    def __init__(self, dim: int, dtype: str = "bf16", capacity: int = 0, device="cuda", *, arg: str = "dtype",
                 held: bool = True):
        self.bytes_per_frame(dim, dtype, arg)
        if dtype == "mx8" and held and dim % 64:
            raise ValueError(f'{arg}="mx8" needs projection_dim % 64 == 0 (MX blocks of 32 over the 2P columns, '
                             f"quantised 128 at a time), got {dim}")
        self.dtype, self.device = dtype, torch.device(device)
        cap = max(int(capacity), 0) if held else 0
        mx8 = dtype == "mx8"
        self.data = torch.empty(cap, 2 * dim, device=self.device, dtype=torch.uint8 if mx8 else BF16)
        self.scales = torch.empty(cap, 2 * dim // 32, device=self.device, dtype=torch.uint8) if mx8 else None

    @staticmethod
    def bytes_per_frame(dim: int, dtype: str = "bf16", arg: str = "dtype") -> int:
        """Bytes per stored row of 2·dim columns: "bf16" 4·dim (3,072 at dim = 768); "mx8" 2·dim e4m3
        bytes + 2·dim/32 E8M0 scale bytes (1,584 at dim = 768, 0.516 of bf16)."""
        if dtype == "bf16":
            return 4 * dim
        if dtype == "mx8":
            return 2 * dim + 2 * dim // 32
        raise ValueError(f"{arg} must be one of {KV_DTYPES}, got {dtype!r}")

    def _buffers(self):
        return ("data",) if self.scales is None else ("data", "scales")

    def reserve(self, rows: int, used: int) -> None:
        """Capacity for rows rows (geometric growth), keeping the first used."""
        if rows <= self.data.shape[0]:
            return
        cap = max(rows, 2 * self.data.shape[0])
        for name in self._buffers():
            old = getattr(self, name)
            grown = torch.empty(cap, old.shape[1], device=self.device, dtype=old.dtype)
            grown[:used].copy_(old[:used])
            setattr(self, name, grown)

    def write(self, at: int, src: torch.Tensor, frames, T: int) -> None:
        """Store the first frames[b] rows of each clip b of src (bf16 [B·T, 2·dim], clip b at rows b·T ..)
        from row at on, back to back; reserve first."""
        parts = (src,) if self.scales is None else ops.mx8_quant(src)
        for part, name in zip(parts, self._buffers()):
            dst = getattr(self, name)
            if all(n == T for n in frames):
                dst[at:at + len(frames) * T].copy_(part)
            else:
                row = at
                for b, n in enumerate(frames):
                    dst[row:row + n].copy_(part[b * T:b * T + n])
                    row += n

    def rows(self, a: int, b: int) -> torch.Tensor:
        """Rows a .. b-1 as bf16: a view for "bf16", what the stored bytes mean (ops.mx8_dequant) for "mx8"."""
        if self.scales is None:
            return self.data[a:b]
        return ops.mx8_dequant(self.data[a:b], self.scales[a:b])

    def xattn_operands(self):
        """k, v, {ks, vs}: the column views ops.xattn_seg_fwd attends over in place."""
        P = self.data.shape[1] // 2
        scales = {} if self.scales is None else dict(ks=self.scales[:, :P // 32], vs=self.scales[:, P // 32:])
        return self.data[:, :P], self.data[:, P:], scales

    def align_operands(self):
        """kv, {scales}: what ops.align_matrix_seg_fwd reads in place."""
        return self.data, ({} if self.scales is None else dict(scales=self.scales))


def kv_bytes_per_frame(dim: int, kv_dtype: str = "bf16") -> int:
    """Bytes an AudioStateStore of projection width dim holds per stored frame (one K|V row of 2·dim
    columns), RowBank.bytes_per_frame: 3,072 at dim = 768 for "bf16", 1,584 for "mx8"."""
    return RowBank.bytes_per_frame(dim, kv_dtype, "kv_dtype")


def align_bytes_per_frame(dim: int, align_dtype: str = "bf16") -> int:
    """Bytes an AudioStateStore(align_rows=True) of projection width dim adds per stored frame, whatever
    kv_dtype is: one K|V row of the alignment head, RowBank.bytes_per_frame."""
    return RowBank.bytes_per_frame(dim, align_dtype, "align_dtype")


class AudioStateStore:
    """What the text -> audio fused pair score needs of every corpus clip, computed once when the
    corpus is indexed: the clip's projection aproj fp32 [P], its unit row (in an
    EmbeddingIndex, for stage 1) and the bf16 text_to_audio_attention K|V rows [frames, 2P] of its
    VALID frames, appended to one growable buffer [capacity, 2P] (geometric growth; reserve_frames
    preallocates) that ste_xattn_seg_fwd attends over in place.  Clip n is the segment of rows
    seg_row[n] .. seg_row[n] + frames[n] - 1.  Dropping the padded frames is exact (§18), so the
    audio mask must be a prefix mask with at least one valid frame, else ValueError.  3 KB per frame
    at P = 768: 1.5 MB per 10 s clip.  Without use_cross_modal only aproj and the unit rows are kept.

    kv_dtype selects how the K|V rows are held (kv_bytes_per_frame):
      "bf16"  kv bf16 [capacity, 2P]: 4P bytes per frame, 3,072 at P = 768 (the default);
      "mx8"   kv uint8 [capacity, 2P] of OCP e4m3 bytes + kv_scales uint8 [capacity, 2P/32] of E8M0
              block scales (one per 32 columns), ops.mx8_quant of each bf16 row as it is added:
              2P + P/16 bytes per frame, 1,584 at P = 768 (0.516 of bf16).  ste_xattn_seg_mx8_fwd
              attends over the bytes in place.  Quantisation is per row, so a clip's bytes depend on
              its bf16 rows alone.  Needs P % 64 == 0, else ValueError.
    kv_rows(n) says what clip n's stored rows mean, as bf16, for either.

    align_rows=True (needs use_word_alignment, else ValueError) also keeps the word-alignment head's
    bf16 K|V rows of the same valid frames in akv [capacity, 2P], row for row beside kv:
    seg_row and frames address both, and ste_align_matrix_seg_fwd reads them in place
    (model.locate_clips).  A clip of more than 2048 valid frames is a ValueError in add.  align_dtype
    selects how these rows are held, independently of kv_dtype (align_bytes_per_frame):
      "bf16"  akv bf16 [capacity, 2P]: 4P more bytes per frame (the default);
      "mx8"   akv uint8 [capacity, 2P] of e4m3 bytes + akv_scales uint8 [capacity, 2P/32] of E8M0 block
              scales, ops.mx8_quant of each bf16 row as it is added: 2P + P/16 more bytes per frame;
              ste_align_matrix_seg_mx8_fwd reads the bytes in place.  Needs P % 64 == 0, else
              ValueError.
    Without align_rows the argument has no effect.  align_kv_rows(n) says what clip n's stored rows
    mean, as bf16, for either.  Both sets of rows are RowBanks, kv_bank and align_bank; kv / kv_scales
    and akv / akv_scales are their tensors.

    add_recording appends one long recording: its frames' rows once, and one entry per
    overlapping window, a view of those rows (so entries may share rows, len() counts windows, and rows /
    nbytes count each frame once; nbytes does not count the 8 bytes per entry of recording_of /
    offset_of).  recording_of / offset_of say which recording an entry belongs to and where in it it
    starts; a clip of add() is a recording of its own at offset 0.

    The store is valid for the weights it was built with: it records the model's
    ParamStore.weights_token() at the first add, and adding to or scoring against it after the
    weights changed raises RuntimeError (check)."""

    def __init__(self, model, device="cuda", index_dtype: torch.dtype = F32, reserve_frames: int = 0,
                 kv_dtype: str = "bf16", align_rows: bool = False, align_dtype: str = "bf16"):
        self.model, self.device = model, torch.device(device)
        self.dim = int(model.projection_dim)
        self.fused = bool(getattr(model, "use_cross_modal", False))
        self.kv_dtype, self.align_dtype = kv_dtype, align_dtype
        self.align_rows = bool(align_rows)
        cap = int(reserve_frames)
        self.kv_bank = RowBank(self.dim, kv_dtype, cap, self.device, arg="kv_dtype", held=self.fused)
        if self.align_rows and not getattr(model, "use_word_alignment", False):
            raise ValueError("align_rows=True needs a model built with use_word_alignment=True")
        # the alignment head's K|V rows (align_rows only), numbered as kv's rows are
        self.align_bank = RowBank(self.dim, align_dtype, cap, self.device, arg="align_dtype", held=self.align_rows)
        self.index = EmbeddingIndex(self.dim, index_dtype, self.device)
        self.rows = 0                         # rows of kv / akv in use
        self._seg_row: list[int] = []
        self._seg_len: list[int] = []
        self._aproj: list[torch.Tensor] = []
        self._dev = None                      # (seg_row int64 [N], frames int32 [N], aproj [N, P]) on the device
        self._token = None
        # add_recording: an entry is a window of a recording; a clip of add() is a recording of its own
        self._rec_of: list[int] = []
        self._off_of: list[int] = []
        self._rec_dev = None                  # (recording_of int32 [N], offset_of int32 [N]) on the device
        self.recordings = 0

    def __len__(self) -> int:
        return len(self._seg_len)

    def check(self) -> None:
        """Raise if the model's weights changed since the store was built."""
        if self._token is not None and self._token != self.model.store.weights_token():
            raise RuntimeError("the AudioStateStore was built with other weights: rebuild it after a weight update")

    @property
    def kv(self) -> torch.Tensor:
        """The K|V rows' buffer [capacity, 2P] (empty without use_cross_modal)."""
        return self.kv_bank.data

    @property
    def kv_scales(self):
        """The E8M0 block scales of kv's rows (kv_dtype "mx8" only, else None)."""
        return self.kv_bank.scales

    @property
    def akv(self):
        """The alignment head's K|V rows [capacity, 2P] (align_rows only, else None)."""
        return self.align_bank.data if self.align_rows else None

    @property
    def akv_scales(self):
        """The E8M0 block scales of akv's rows (align_rows with align_dtype "mx8" only, else None)."""
        return self.align_bank.scales if self.align_rows else None

    def _reserve(self, rows: int) -> None:
        if self.align_rows:
            self.align_bank.reserve(rows, self.rows)
        if self.fused:
            self.kv_bank.reserve(rows, self.rows)

    @torch.no_grad()
    def add(self, input_values, attention_mask_audio=None, *, audio_encoded=None) -> None:
        """Append a batch of clips: one model.encode_audio pass in eval arithmetic (or its result
        audio_encoded = (projection, hidden)), one K/V projection, one device -> host sync (the
        frame counts and the mask check)."""
        model, eng = self.model, self.model.engine
        self.check()
        if audio_encoded is None:
            with model._eval_arithmetic():
                audio_encoded = model.encode_audio(input_values, attention_mask_audio)
        aproj, ah = audio_encoded
        B, T, Ha = ah.shape
        am32 = eng._frame_mask32(attention_mask_audio, B, T)
        if am32 is None:
            frames = [T] * B
        else:
            fm = am32.view(B, T) != 0
            bad = (fm[:, 1:] & ~fm[:, :-1]).any() | (~fm.any(1)).any()
            *frames, bad = torch.cat([fm.sum(1), bad.view(1).to(torch.int64)]).tolist()
            if bad:
                raise ValueError("AudioStateStore.add needs prefix audio masks with at least one valid frame per clip")
        if self.align_rows and max(frames) > ALIGN_MAX_FRAMES:
            raise ValueError(f"align_rows=True holds clips of at most {ALIGN_MAX_FRAMES} valid frames "
                             f"(the alignment kernels' limit), got {max(frames)}")
        if self.fused or self.align_rows:
            model.store.sync_shadow()
            ahb = ops.cast_bf16(ah.reshape(B * T, Ha).float().contiguous(),
                                torch.empty(B * T, Ha, device=self.device, dtype=BF16))
            self._reserve(self.rows + sum(frames))
            if self.fused:
                kv = eng._kv("text_to_audio_attention", "audio_seq_to_projection", ahb)[0]
            if self.align_rows:
                from .align import audio_kv
                akv = audio_kv(eng, ahb)
            if self.fused:                     # both projections first, then the copies, bank by bank
                self.kv_bank.write(self.rows, kv, frames, T)
            if self.align_rows:
                self.align_bank.write(self.rows, akv, frames, T)
        for n in frames:
            self._seg_row.append(self.rows)
            self._seg_len.append(n)
            self.rows += n
            self._rec_of.append(self.recordings)
            self._off_of.append(0)
            self.recordings += 1
        aproj = aproj.detach().float()
        self._aproj.append(aproj.clone())
        self.index.add(_unit_rows(aproj))
        self._dev = self._rec_dev = None
        if self._token is None:
            self._token = model.store.weights_token()

    @torch.no_grad()
    def add_recording(self, input_values, *, window_frames: int = 1500, hop_frames: int = 750,
                      chunk_frames: int = 1000, context_frames: int = 250, chunk_batch: int = 8) -> int:
        """Append ONE long recording and return its recording id.  input_values: its w2v-bert
        features [F, 160] (or [1, F, 160]), every frame valid.  plan_recording says how: the encoder runs
        chunk by chunk (engine.audio_forward in eval arithmetic on batches of chunk_batch chunk inputs,
        right-padded under a prefix mask; each chunk keeps its own frames and drops the context), the
        K|V rows and the alignment rows of the F kept frames are appended ONCE, back to back, and every
        window becomes one ordinary entry of the store: a VIEW of those rows (seg_row = the recording's
        first row + the window's start, frames = its length), with its own aproj and unit row, pooled
        from the recording's hidden states in place by ops.attn_pool_seg_fwd.  So len(store) counts
        windows, rows and nbytes count each frame once, and search, score_clips, rerank_clips, locate_clips,
        kv_rows(n) and align_kv_rows(n) take window ids unchanged; recording_of / offset_of map a window
        back (retrieval.search_recordings).  The defaults make the largest encoder input 1500 frames.

        ValueError, before anything is appended: a raw-waveform (wav2vec2) model, a model without
        use_attentive_pooling, plan_recording's refusals, window_frames over 2048 with align_rows.
        RuntimeError if the weights changed (check)."""
        model, eng = self.model, self.model.engine
        if eng.raw_audio:
            raise ValueError("add_recording takes w2v-bert features; a raw-waveform (wav2vec2) model is not supported")
        if not model.use_attentive_pooling:
            raise ValueError("add_recording needs a model built with use_attentive_pooling=True")
        x = input_values
        if x.dim() == 3 and x.shape[0] == 1:
            x = x[0]
        if x.dim() != 2:
            raise ValueError(f"add_recording takes the features [F, 160] of ONE recording, got {tuple(input_values.shape)}")
        if int(chunk_batch) < 1:
            raise ValueError(f"chunk_batch must be at least 1, got {chunk_batch}")
        F, fin = x.shape
        plan = plan_recording(F, window_frames, hop_frames, chunk_frames, context_frames,
                              max_window=ALIGN_MAX_FRAMES if self.align_rows else POOL_MAX_FRAMES)
        self.check()
        model.store.sync_shadow()
        x = x.to(self.device).contiguous()
        D = eng.acfg.hidden_size
        h = torch.empty(F, D, device=self.device, dtype=F32)          # the kept frames' states
        hs = torch.empty(F, 2 * D, device=self.device, dtype=BF16)    # and their [hi | lo] split image
        chunks = list(zip(plan["keep"], plan["input"]))
        for c0 in range(0, len(chunks), int(chunk_batch)):
            part = chunks[c0:c0 + int(chunk_batch)]
            T = max(ib - ia for _, (ia, ib) in part)
            feats = x.new_zeros(len(part), T, fin)
            mask = torch.zeros(len(part), T, dtype=torch.int64, device=self.device)
            for j, (_, (ia, ib)) in enumerate(part):
                feats[j, :ib - ia] = x[ia:ib]
                mask[j, :ib - ia] = 1
            ctx = {}
            hc, _ = eng.audio_forward(feats, mask, False, 0, ctx, save=False)
            for j, ((ka, kb), (ia, _)) in enumerate(part):
                r = j * T + ka - ia
                h[ka:kb] = hc[r:r + kb - ka]
                hs[ka:kb] = ctx["a_hs"][r:r + kb - ka]
        base = self.rows
        if self.fused or self.align_rows:
            hb = ops.cast_bf16(h, torch.empty(F, D, device=self.device, dtype=BF16))
            self._reserve(base + F)
            if self.fused:
                self.kv_bank.write(base, eng._kv("text_to_audio_attention", "audio_seq_to_projection", hb)[0], [F], F)
            if self.align_rows:
                from .align import audio_kv
                self.align_bank.write(base, audio_kv(eng, hb), [F], F)
        starts, lens = plan["window_start"], plan["window_len"]
        pooled = eng._pool_seg_fwd("audio_pooling", h, hs, torch.tensor(starts, dtype=torch.int64, device=self.device),
                                   torch.tensor(lens, dtype=I32, device=self.device))
        aproj = eng._proj_fwd("audio_projection", pooled, len(starts), False, 0, {})
        rec = self.recordings
        for s, n in zip(starts, lens):
            self._seg_row.append(base + s)
            self._seg_len.append(n)
            self._rec_of.append(rec)
            self._off_of.append(s)
        self.rows += F
        self.recordings += 1
        self._aproj.append(aproj.clone())
        self.index.add(_unit_rows(aproj))
        self._dev = self._rec_dev = None
        if self._token is None:
            self._token = model.store.weights_token()
        return rec

    def _rec_tables(self):
        if self._rec_dev is None:
            self._rec_dev = (torch.tensor(self._rec_of, dtype=I32, device=self.device),
                             torch.tensor(self._off_of, dtype=I32, device=self.device))
        return self._rec_dev

    @property
    def recording_of(self) -> torch.Tensor:
        """int32 [N]: the recording each entry (window) belongs to; a clip of add() is a recording of its own."""
        return self._rec_tables()[0]

    @property
    def offset_of(self) -> torch.Tensor:
        """int32 [N]: the entry's first frame inside its recording (0 for a clip of add())."""
        return self._rec_tables()[1]

    def _tables(self):
        if self._dev is None:
            self._dev = (torch.tensor(self._seg_row, dtype=torch.int64, device=self.device),
                         torch.tensor(self._seg_len, dtype=I32, device=self.device),
                         torch.cat(self._aproj) if self._aproj else torch.empty(0, self.dim, device=self.device))
            self._aproj = [self._dev[2]] if self._aproj else []
        return self._dev

    @property
    def seg_row(self) -> torch.Tensor:
        """int64 [N]: the first row of each clip's K/V in kv."""
        return self._tables()[0]

    @property
    def frames(self) -> torch.Tensor:
        """int32 [N]: the valid frames (stored K/V rows) of each clip."""
        return self._tables()[1]

    @property
    def aproj(self) -> torch.Tensor:
        """fp32 [N, P]: the clips' projections."""
        return self._tables()[2]

    @property
    def nbytes(self) -> int:
        """Bytes held for the clips added so far (the K/V rows in use, aproj, the unit rows and the segment table)."""
        n = len(self)
        return (self.rows * kv_bytes_per_frame(self.dim, self.kv_dtype) + n * self.dim * 4
                + n * self.dim * (2 if self.index.dtype == BF16 else 4) + n * 12
                + (self.rows * align_bytes_per_frame(self.dim, self.align_dtype) if self.align_rows else 0))

    def kv_rows(self, n: int) -> torch.Tensor:
        """Clip n's stored K|V rows as bf16 [frames, 2P]: a slice of kv for "bf16" (a view), what the
        stored bytes mean (ops.mx8_dequant) for "mx8"."""
        if not self.fused:
            raise ValueError("the store keeps no K/V rows without use_cross_modal")
        return self.kv_bank.rows(self._seg_row[n], self._seg_row[n] + self._seg_len[n])

    def align_kv_rows(self, n: int) -> torch.Tensor:
        """Clip n's stored alignment-head K|V rows as bf16 [frames, 2P]: a slice of akv for "bf16" (a
        view), what the stored bytes mean (ops.mx8_dequant) for "mx8"."""
        if not self.align_rows:
            raise ValueError("the store keeps no alignment rows without align_rows=True")
        return self.align_bank.rows(self._seg_row[n], self._seg_row[n] + self._seg_len[n])

    def search(self, text_emb: torch.Tensor, k: int):
        """Stage 1: (values fp32 [Q, k], indices int32 [Q, k]) of the k best clips per unit text row,
        as EmbeddingIndex.search."""
        return self.index.search(text_emb, k)


@torch.no_grad()
def rerank_clips(model, input_ids, attention_mask, store, idx, *, text_encoded=None):
    """Rerank each text query's retrieved clips idx [Q, k] (clip ids of an AudioStateStore, as
    returned by store.search) with the fused pair score: model.score_clips -> rerank_order.
    Returns (values fp32 [Q, k], indices [Q, k]).  text_encoded: see score_clips."""
    scores = model.score_clips(input_ids, attention_mask, store, idx, text_encoded=text_encoded)
    return rerank_order(scores, torch.as_tensor(idx).to(scores.device))


@torch.no_grad()
def search_clips(model, store, input_ids, attention_mask, k, *, rerank=True, locate=True, word_ids=None,
                 free_ends=False, spot_bias=0.0):
    """A typed phrase against an indexed archive, end to end: ONE text-encoder pass per
    query, shared by store.search (stage 1), rerank_clips (stage 2, with rerank=True and a
    use_cross_modal model) and model.locate_clips (where in each hit the phrase is spoken, with
    locate=True; needs a store built with align_rows=True).  Returns (values fp32 [Q, k], indices
    [Q, k], location): the hits in their final (reranked) order and model.locate_clips' dict for
    exactly those indices, None with locate=False.  free_ends / spot_bias go to model.locate_clips:
    with free_ends=True the phrase is located as a fragment of what each hit says."""
    if attention_mask is None:
        attention_mask = torch.ones_like(input_ids)
    with model._eval_arithmetic():
        enc = model.encode_text(input_ids, attention_mask)
    vals, idx = store.search(_unit_rows(enc[0]), k)
    if rerank and getattr(model, "use_cross_modal", False):
        vals, idx = rerank_clips(model, input_ids, attention_mask, store, idx, text_encoded=enc)
    where = model.locate_clips(input_ids, attention_mask, store, idx, word_ids=word_ids, text_encoded=enc,
                               free_ends=free_ends, spot_bias=spot_bias) if locate else None
    return vals, idx, where


def _same_recording(store, win, other):
    """other where it is a window of win's recording, else -1 (win, other int [Q, k]; -1 = none)."""
    N = len(store)
    ok = (win >= 0) & (other >= 0) & (other < N)
    rec = store.recording_of
    ok = ok & (rec[win.clamp(min=0).long()] == rec[other.clamp(0, max(N - 1, 0)).long()])
    return torch.where(ok, other, torch.full_like(other, -1))


@torch.no_grad()
def search_recordings(model, store, input_ids, attention_mask, k, *, window_k=None, rerank=True, locate=True,
                      neighbours=True, free_ends=True, spot_bias=0.0, word_ids=None):
    """A typed phrase against an archive of long recordings (AudioStateStore.add_recording):
    search_clips over the store's windows, reduced to one hit per recording and reported in recording
    time.  ONE text-encoder pass per query, shared by every stage.  Stage 1 searches m = window_k or
    min(4·k, 128, len(store)) windows (128: the top-k kernel's limit); with rerank=True and a
    use_cross_modal model rerank_clips reorders them; best_per_recording keeps each recording's best
    window.  Returns (values fp32 [Q, k], recordings [Q, k], windows [Q, k], location), empty slots
    (-inf, -1, -1); location is None with locate=False.

    locate=True (needs a store built with align_rows=True) runs model.locate_clips on the chosen windows
    (free_ends / spot_bias as in search_clips; the default here is the free-endpoint decode, since a
    window rarely holds exactly the phrase).  neighbours=True (with free_ends=True only) also locates
    the previous and the next window OF THE SAME RECORDING, in one locate_clips call on [Q, 3k]
    candidates (centre | previous | next, -1 where there is none), and keeps per hit the window with the
    largest path_score, the first maximum in that order winning; `windows` reports the window kept.
    location is locate_clips' dict for the kept windows plus recording_hit_spans / recording_hit_seconds
    and recording_token_spans / recording_token_seconds: the window-local values moved by the window's
    offset_of (times engine.frame_seconds), (-1, -1) kept."""
    if attention_mask is None:
        attention_mask = torch.ones_like(input_ids)
    k = int(k)
    m = int(window_k) if window_k else min(4 * k, 128, len(store))
    with model._eval_arithmetic():
        enc = model.encode_text(input_ids, attention_mask)
    vals, idx = store.search(_unit_rows(enc[0]), max(m, 1))
    if rerank and getattr(model, "use_cross_modal", False):
        vals, idx = rerank_clips(model, input_ids, attention_mask, store, idx, text_encoded=enc)
    vals, recs, wins = best_per_recording(vals, idx, store.recording_of, k)
    if not locate:
        return vals, recs, wins, None
    kw = dict(word_ids=word_ids, text_encoded=enc, free_ends=free_ends, spot_bias=spot_bias)
    if neighbours and free_ends:
        cand = torch.cat([wins, _same_recording(store, wins, wins - 1), _same_recording(store, wins, wins + 1)], 1)
        where3 = model.locate_clips(input_ids, attention_mask, store, cand, **kw)
        Q = wins.shape[0]
        pc, pl, pr = where3["path_score"].view(Q, 3, k).unbind(1)
        sel = (pl > pc).long()                                       # centre, unless the previous window beats it,
        sel = torch.where(pr > torch.maximum(pc, pl), 2, sel)        # unless the next one beats both
        wins = cand.view(Q, 3, k).gather(1, sel.view(Q, 1, k).to(cand.device)).squeeze(1)
        where = {}
        for key, v in where3.items():
            v = v.view(Q, 3, k, *v.shape[2:])
            pick = sel.view(Q, 1, k, *([1] * (v.dim() - 3))).expand(Q, 1, k, *v.shape[3:])
            where[key] = v.gather(1, pick).squeeze(1)
    else:
        where = model.locate_clips(input_ids, attention_mask, store, wins, **kw)
    off = torch.where(wins >= 0, store.offset_of[wins.clamp(min=0).long()], 0).to(I32)
    fs = model.engine.frame_seconds
    for name, o in (("hit", off.view(*off.shape, 1)), ("token", off.view(*off.shape, 1, 1))):
        spans = where[name + "_spans"]
        where[f"recording_{name}_spans"] = torch.where(spans < 0, spans, spans + o)
        secs = where[name + "_seconds"]
        where[f"recording_{name}_seconds"] = torch.where(spans < 0, secs, secs + o.float() * fs)
    return vals, recs, wins, where


def _pad_rows(chunks, fill):
    """Concatenate [n_i, L_i] chunks, right-padded to the longest L with fill."""
    L = max(c.shape[1] for c in chunks)
    return torch.cat([torch.nn.functional.pad(c, (0, L - c.shape[1]), value=fill) for c in chunks])


@torch.no_grad()
def evaluate_retrieval(model, data_loader, device, ks=(1, 5, 10), index_dtype: torch.dtype = F32,
                       return_ranks: bool = False, rerank_k: int = 0, rerank_t2a: bool = False,
                       store_kv_dtype: str = "bf16") -> dict:
    """One pass over a loader of the reference's batch dicts (custom_collate_fn's keys): embeds the
    clean transcripts and the audio, indexes both and ranks pair i's partner for query i in both
    directions.  Returns {"a2t": retrieval_metrics, "t2a": retrieval_metrics} (audio -> text,
    text -> audio), plus the rank tensors under "a2t_ranks" / "t2a_ranks" on request.  None
    batches are skipped, as evaluate() does; everything stays on the device until the metrics are
    read.

    rerank_k > 0 with a use_cross_modal model adds "a2t_rerank" (and "a2t_rerank_ranks"): the first
    pass also keeps the clean transcripts' token ids and masks on the device (right-padded to the
    longest L with the pad id and mask 0, which leaves a transcript's states unchanged), and the
    loader is iterated a SECOND time: per batch the audio is encoded once, its rerank_k best
    transcripts are searched and reranked with the fused pair score (rerank), and the pair's rank
    becomes its position in that list when it is among them.  The second pass must yield the same
    items in the same order (a loader with shuffle=False over a deterministic dataset); each
    batch's input_ids_pos is compared with the stored rows and a mismatch raises ValueError.

    rerank_t2a=True (with rerank_k > 0 and a use_cross_modal model) adds "t2a_rerank" (and
    "t2a_rerank_ranks"), the other direction: the first pass also fills an AudioStateStore with the
    clips' audio states, and after it each batch of clean transcripts (the kept token rows) is
    reranked against store.search(text_emb, rerank_k) with rerank_clips.  This direction needs no
    further loader pass.  With the flag off nothing changes.  store_kv_dtype is that store's kv_dtype
    ("bf16", or "mx8" for MX-fp8 rows at about half the bytes).
    Out of scope: the model_infer.py variant, a cache of the corpus text K/V, and any backward."""
    model.eval()
    do_rerank = rerank_k > 0 and getattr(model, "use_cross_modal", False)
    do_t2a = do_rerank and rerank_t2a
    store = None
    texts, audios, tok_ids, tok_mask = [], [], [], []
    text_index = audio_index = None

    def on_device(batch):
        return {k: v.to(device, non_blocking=True) if isinstance(v, torch.Tensor) else v for k, v in batch.items()}

    for batch in data_loader:
        if batch is None:
            continue
        b = on_device(batch)
        t = embed_texts(model, b["input_ids_pos"], b["attention_mask_pos"])
        if do_t2a:
            enc = model.encode_audio(b["input_values"], b.get("attention_mask_audio"))
            a = _unit_rows(enc[0])
            if store is None:
                store = AudioStateStore(model, a.device, index_dtype, kv_dtype=store_kv_dtype)
            store.add(b["input_values"], b.get("attention_mask_audio"), audio_encoded=enc)   # indexes a as well
        else:
            a = embed_audio(model, b["input_values"], b.get("attention_mask_audio"))
        if text_index is None:
            text_index = EmbeddingIndex(t.shape[1], index_dtype, t.device)
            audio_index = store.index if do_t2a else EmbeddingIndex(a.shape[1], index_dtype, a.device)
        text_index.add(t)
        if not do_t2a:
            audio_index.add(a)
        texts.append(t)
        audios.append(a)
        if do_rerank:
            tok_ids.append(b["input_ids_pos"])
            tok_mask.append(b["attention_mask_pos"])
    if text_index is None:
        a2t = t2a = torch.empty(0, dtype=torch.int64)
    else:
        pair = torch.arange(len(text_index), device=text_index.device, dtype=I32)
        a2t = text_index.ranks(torch.cat(audios), pair)
        t2a = audio_index.ranks(torch.cat(texts), pair)
    out = {"a2t": retrieval_metrics(a2t, ks), "t2a": retrieval_metrics(t2a, ks)}
    if return_ranks:
        out.update(a2t_ranks=a2t, t2a_ranks=t2a)
    if not do_rerank:
        return out
    reranked = [a2t[:0]]
    if text_index is not None:
        ids = _pad_rows(tok_ids, model.text_cfg.pad_token_id)
        mask = _pad_rows(tok_mask, 0)
    if do_t2a:
        rr, at = [t2a[:0]], 0
        for t in texts:                # the first pass's batches of clean transcripts
            nb = t.shape[0]
            idx = store.search(t, rerank_k)[1]
            order = rerank_clips(model, ids[at:at + nb], mask[at:at + nb], store, idx)[1]
            tgt = torch.arange(at, at + nb, device=idx.device, dtype=idx.dtype)
            rr.append(reranked_ranks(t2a[at:at + nb], idx, order, tgt))
            at += nb
        rr = torch.cat(rr)
        out["t2a_rerank"] = retrieval_metrics(rr, ks)
        if return_ranks:
            out["t2a_rerank_ranks"] = rr
    if text_index is not None:
        n, at = len(text_index), 0
        for batch in data_loader:
            if batch is None:
                continue
            b = on_device(batch)
            bi = b["input_ids_pos"]
            nb, Lb = bi.shape
            if at + nb > n or Lb > ids.shape[1] or not torch.equal(bi, ids[at:at + nb, :Lb]) \
                    or bool(mask[at:at + nb, Lb:].any()):
                raise ValueError("evaluate_retrieval(rerank_k>0): the loader's second pass differs from its first "
                                 f"at items {at}..{at + nb - 1}; it must yield the same items in the same order "
                                 "(shuffle=False)")
            am = b.get("attention_mask_audio")
            enc = model.encode_audio(b["input_values"], am)
            idx = text_index.search(_unit_rows(enc[0]), rerank_k)[1]
            order = rerank(model, b["input_values"], am, ids, mask, idx, audio_encoded=enc)[1]
            tgt = torch.arange(at, at + nb, device=idx.device, dtype=idx.dtype)
            reranked.append(reranked_ranks(a2t[at:at + nb], idx, order, tgt))
            at += nb
        if at != n:
            raise ValueError(f"evaluate_retrieval(rerank_k>0): the second pass yielded {at} items, the first {n}")
    rr = torch.cat(reranked)
    out["a2t_rerank"] = retrieval_metrics(rr, ks)
    if return_ranks:
        out["a2t_rerank_ranks"] = rr
    return out
