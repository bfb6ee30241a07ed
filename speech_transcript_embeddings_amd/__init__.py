"""MI355X-native speech<->transcript contrastive training step.

A from-scratch gfx950 implementation of the hot path of
yuriyvnv/speech_transcript_embeddings (training/trainer_unfreeze.py:train_epoch):
GPU fbank -> w2v-bert Conformer + XLM-R encoders -> pooling / projection /
cross-modal heads -> AlignmentAwareInfoNCE -> backward -> clip -> AdamW, with
every hot op a hand-written HIP kernel in libste.so (include/ste.h).
"""
__version__ = "0.2.0"

from . import torch_ops  # noqa: E402,F401  (torch.ops.ste.* custom operators)
from .retrieval import (AudioStateStore, EmbeddingIndex, best_per_recording, embed_audio, embed_texts,  # noqa: E402,F401
                        evaluate_retrieval, plan_candidates, plan_clip_pairs, plan_recording, rerank, rerank_clips,
                        rerank_order, reranked_ranks, retrieval_metrics, search_clips, search_recordings)
