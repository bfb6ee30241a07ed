"""Word timestamps without a GPU: the references of tests/kref_align.py pinned to
torch.nn.MultiheadAttention and to a brute-force enumeration of every monotone path, the two new
ste:: ops' schemas and fake implementations, the C ABI of the two entry points (declared, exported,
in the ctypes table, contract violations returned before any launch), words_from_tokens on a
hand-written case and Engine.frame_seconds."""
import ctypes as C
import math

import numpy as np
import pytest
import torch
from torch._subclasses.fake_tensor import FakeTensorMode

from kref_align import (align_matrix_ref, monotone_paths, path_score, planted, viterbi_batch_ref, viterbi_ref)
from speech_transcript_embeddings_amd import torch_ops
from speech_transcript_embeddings_amd.align import words_from_tokens

ERR_ARG, ERR_SHAPE = 1001, 1002


# ------------------------------------------------------------------ references
@pytest.mark.parametrize("masked", [False, True])
def test_align_matrix_ref_is_multihead_attention(masked):
    """align_matrix_ref against nn.MultiheadAttention(batch_first, need_weights, per-head weights)
    .mean(1) with key_padding_mask in float64, the same in-projection loaded into the module."""
    torch.manual_seed(3)
    B, L, T, P, nh = 2, 5, 11, 32, 4
    mha = torch.nn.MultiheadAttention(P, nh, batch_first=True).double()
    with torch.no_grad():
        mha.in_proj_bias.normal_()
        mha.out_proj.weight.copy_(torch.eye(P))
        mha.out_proj.bias.zero_()
    xt, xa = torch.randn(B, L, P).double(), torch.randn(B, T, P).double()
    kmask = None
    if masked:
        kmask = torch.ones(B, T, dtype=torch.int32)
        kmask[1, 7:] = 0
    with torch.no_grad():
        out, w = mha(xt, xa, xa, key_padding_mask=None if kmask is None else kmask == 0, need_weights=True,
                     average_attn_weights=False)
        W, bW = mha.in_proj_weight, mha.in_proj_bias
        q = xt.reshape(B * L, P) @ W[:P].T + bW[:P]
        kv = xa.reshape(B * T, P) @ W[P:].T + bW[P:]
    m, o = align_matrix_ref(q, kv, None if kmask is None else kmask.view(-1), B, L, T, P, nh)
    assert w.shape == (B, nh, L, T)
    assert float((m - w.mean(1)).abs().max()) < 1e-14
    assert float((o - out.reshape(B * L, P)).abs().max()) < 1e-13
    if masked:
        assert float(m[1, :, 7:].abs().max()) == 0.0


@pytest.mark.parametrize("L,T,n,F", [(1, 1, 1, 1), (5, 5, 5, 5), (7, 40, 6, 33), (64, 499, 64, 499),
                                     (65, 130, 65, 129), (256, 1500, 200, 1499)])
def test_viterbi_ref_recovers_planted_paths(L, T, n, F):
    e, want = planted(L, T, n, F, seed=L + T)
    spans, score, path = viterbi_ref(e, n, F)
    assert np.array_equal(spans, want) and score == 0.0
    assert path[0] == 0 and path[-1] == n - 1 and set(np.diff(path)) <= {0, 1}


def test_viterbi_ref_ties_advance_earliest():
    spans, score, _ = viterbi_ref(np.zeros((6, 3), dtype=np.float32), 3, 6)
    assert spans.tolist() == [[0, 1], [1, 2], [2, 6]] and score == 0.0


def test_viterbi_ref_against_all_paths():
    """n <= 5, F <= 9, integer emissions (every sum exact, many ties) and N(0,1) floats: the score is
    the best over all C(F-1, n-1) monotone paths and the returned path attains it."""
    rng = np.random.default_rng(11)
    for n in range(1, 6):
        for F in range(n, 10):
            for kind in ("int", "float"):
                e = (rng.integers(-8, 1, (F, n)).astype(np.float32) if kind == "int"
                     else rng.standard_normal((F, n)).astype(np.float32))
                spans, score, path = viterbi_ref(e, n, F)
                scores = [path_score(e, p) for p in monotone_paths(n, F)]
                assert len(scores) == math.comb(F - 1, n - 1)
                assert score == max(scores), (n, F, kind)
                assert path_score(e, path) == score
                assert spans[0, 0] == 0 and spans[-1, 1] == F and np.array_equal(spans[1:, 0], spans[:-1, 1])
                assert (spans[:, 1] > spans[:, 0]).all()


def test_viterbi_batch_ref_conventions():
    e = np.zeros((3, 6, 4), dtype=np.float32)
    spans, score = viterbi_batch_ref(e, [3, 5, 4], [6, 6, 3], 4)
    assert spans[0].tolist() == [[0, 1], [1, 2], [2, 6], [-1, -1]] and score[0] == 0.0
    assert (spans[1:] == -1).all() and np.isneginf(score[1:]).all()      # n > L; F < n


# ------------------------------------------------------------------ torch ops
def test_ops_schemas_and_fakes():
    assert "align_matrix" in torch_ops.OPS and "align_decode" in torch_ops.OPS
    s = str(torch.ops.ste.align_matrix.default._schema)
    assert s.startswith("ste::align_matrix(Tensor q, Tensor kv, Tensor? kmask, ") and s.endswith(
        "-> (Tensor, Tensor, Tensor)"), s
    s = str(torch.ops.ste.align_decode.default._schema)
    assert s == "ste::align_decode(Tensor emit, Tensor ntok, Tensor nfrm) -> (Tensor, Tensor)", s
    with FakeTensorMode():
        B, L, T, P = 3, 12, 49, 128
        q, kv = torch.empty(B, L, P, dtype=torch.bfloat16), torch.empty(B, T, 2 * P, dtype=torch.bfloat16)
        for km in (None, torch.empty(B, T, dtype=torch.int32)):
            m, e, o = torch.ops.ste.align_matrix(q, kv, km, 4)
            assert m.shape == (B, L, T) and m.dtype == torch.float32
            assert e.shape == (B, T, L) and e.dtype == torch.float32
            assert o.shape == (B, L, P) and o.dtype == torch.bfloat16
        n = torch.empty(B, dtype=torch.int32)
        spans, score = torch.ops.ste.align_decode(e, n, n)
        assert spans.shape == (B, L, 2) and spans.dtype == torch.int32
        assert score.shape == (B,) and score.dtype == torch.float32


# ------------------------------------------------------------------ C ABI
def test_symbols_declared_exported_and_bound():
    from pathlib import Path

    from speech_transcript_embeddings_amd import _lib
    header = (Path(__file__).resolve().parents[1] / "include" / "ste.h").read_text()
    for name, nargs in (("ste_align_matrix_fwd", 16), ("ste_align_decode", 10)):
        assert f"int {name}(" in header
        assert name in _lib.SYMBOLS and len(_lib._SIGS[name][1]) == nargs and _lib._SIGS[name][0] is C.c_int
        assert _lib.fn(name) is not None                     # exported by libste.so


def test_argument_errors_return_status_without_launch():
    """No GPU here: a launch would fail differently.  Pointers are never dereferenced."""
    from speech_transcript_embeddings_amd import _lib
    mat, dec = _lib.fn("ste_align_matrix_fwd"), _lib.fn("ste_align_decode")
    A = 1 << 20

    def call_mat(B=2, L=9, T=17, P=32, nh=4, matrix=A, emit=A, lde=None, out=A):
        return mat(A, P, A, 2 * P, None, B, L, T, P, nh, matrix, emit, L if lde is None else lde, out, P, None)

    assert call_mat(matrix=None, emit=None, out=None) == ERR_ARG     # nothing asked for
    assert call_mat(T=2049) == ERR_SHAPE
    assert call_mat(P=48, nh=4) == ERR_SHAPE                         # d = 12: d % 8 != 0
    assert call_mat(P=2048, nh=4) == ERR_SHAPE                       # d = 512 > 256
    assert call_mat(P=34, nh=4) == ERR_SHAPE                         # P % nh != 0
    assert call_mat(lde=8) == ERR_SHAPE                              # lde < L
    for z in ("B", "L", "T"):
        assert call_mat(**{z: 0}) == ERR_SHAPE, z

    def call_dec(B=2, L=9, T=17, lde=None, emit=A, spans=A, score=A):
        return dec(emit, L if lde is None else lde, A, A, B, L, T, spans, score, None)

    assert call_dec(L=257) == ERR_SHAPE
    assert call_dec(T=2049) == ERR_SHAPE
    assert call_dec(lde=8) == ERR_SHAPE
    for z in ("B", "L", "T"):
        assert call_dec(**{z: 0}) == ERR_SHAPE, z
    for z in ("emit", "spans", "score"):
        assert call_dec(**{z: None}) == ERR_ARG, z


# ------------------------------------------------------------------ words
def test_words_from_tokens_hand_case():
    """Row 0: <s>, a two-token word 0, word 2 (word id 1 is never used: a gap), </s>, one padding
    token.  Row 1: <s>, word 0, </s> and padding, so its words 1 and 2 are empty."""
    spans = torch.tensor([[[0, 3], [3, 5], [5, 9], [9, 12], [12, 20], [-1, -1]],
                          [[0, 1], [1, 7], [7, 8], [-1, -1], [-1, -1], [-1, -1]]], dtype=torch.int32)
    scores = torch.tensor([[0.5, 1.0, 2.0, 4.0, 0.25, 0.0], [0.5, 3.0, 0.25, 0.0, 0.0, 0.0]])
    wid = torch.tensor([[-1, 0, 0, 2, -1, -1], [-1, 0, -1, -1, -1, -1]])
    ws, wsc = words_from_tokens(spans, scores, wid)
    assert ws.dtype == torch.int32 and ws.shape == (2, 3, 2) and wsc.shape == (2, 3)
    assert ws.tolist() == [[[3, 9], [-1, -1], [9, 12]], [[1, 7], [-1, -1], [-1, -1]]]
    assert wsc.tolist() == [[1.5, 0.0, 4.0], [3.0, 0.0, 0.0]]
    # a word id on a token without a span (beyond the decoded tokens) does not count
    wid2 = wid.clone()
    wid2[1, 4] = 1
    ws2, wsc2 = words_from_tokens(spans, scores, wid2)
    assert ws2.tolist() == ws.tolist() and wsc2.tolist() == wsc.tolist()
    ws3, wsc3 = words_from_tokens(spans, scores, torch.full((2, 6), -1))
    assert ws3.shape == (2, 0, 2) and wsc3.shape == (2, 0)


# ------------------------------------------------------------------ frame hop
def test_frame_seconds_from_the_configurations():
    from types import SimpleNamespace

    from speech_transcript_embeddings_amd.engine import Engine
    from speech_transcript_embeddings_amd.modules import AudioConfig, W2V2Config
    for cfg in (AudioConfig(), W2V2Config()):
        assert Engine.frame_seconds.fget(SimpleNamespace(acfg=cfg, raw_audio=isinstance(cfg, W2V2Config))) == 0.02
    half = W2V2Config(conv_stride=(5, 2, 2, 2, 2, 2, 1))
    assert Engine.frame_seconds.fget(SimpleNamespace(acfg=half, raw_audio=True)) == 0.01
