"""References for the word-timestamp kernels: the head-averaged alignment matrix in the
reference's own expression, and the monotone decode in numpy float32 with exactly the recurrence
and tie rule of include/ste.h.  tests/test_align_cpu.py pins both: the matrix to
torch.nn.MultiheadAttention, the decode to a brute-force enumeration of every monotone path."""
import itertools

import numpy as np
import torch

F32_MIN = float(np.finfo(np.float32).tiny)   # FLT_MIN


def align_matrix_ref(q, kv, kmask, B, L, T, P, nh, dt=torch.float64):
    """q [B*L, P], kv [B*T, 2P] = [K | V], kmask [B*T] (0 = padded key) or None, evaluated in dtype dt
    on the CPU -> (matrix [B, L, T] = softmax(q_h·k_h/√d).mean(heads), out [B*L, P])."""
    d = P // nh
    q, kv = q.detach().cpu().to(dt), kv.detach().cpu().to(dt)
    qh = q.reshape(B, L, nh, d).transpose(1, 2)
    kh, vh = (x.reshape(B, T, nh, d).transpose(1, 2) for x in (kv[:, :P], kv[:, P:2 * P]))
    s = (qh @ kh.transpose(-1, -2)) / (d ** 0.5)
    if kmask is not None:
        s = s.masked_fill(kmask.detach().cpu().view(B, 1, 1, T) == 0, float("-inf"))
    p = s.softmax(-1)
    return p.mean(1), (p @ vh).transpose(1, 2).reshape(B * L, P)


def emit_ref(matrix):
    """log(max(matrix, FLT_MIN)) in float64, frame-major [B, T, L]."""
    return matrix.detach().cpu().double().clamp_min(F32_MIN).log().transpose(1, 2).contiguous()


def viterbi_ref(e, n, F):
    """One pair.  e float32 [T, >= n] frame-major emissions, n tokens, F frames ->
    (spans int32 [n, 2] as (first frame, last frame + 1), score float32, path int [F]).
    D_0[0] = e[0][0], D_0[l>0] = -inf; D_t[l] = (D_{t-1}[l-1] > D_{t-1}[l] ? D_{t-1}[l-1] : D_{t-1}[l])
    + e[t][l], one float32 add per cell, the path advancing only on a strict improvement; the walk
    back starts at (F-1, n-1)."""
    e = np.asarray(e, dtype=np.float32)
    assert 1 <= n <= e.shape[1] and n <= F <= e.shape[0]
    D = np.full(n, -np.inf, dtype=np.float32)
    D[0] = e[0, 0]
    adv = np.zeros((F, n), dtype=bool)
    with np.errstate(invalid="ignore"):
        for t in range(1, F):
            left = np.concatenate([np.float32([-np.inf]), D[:-1]])
            a = left > D
            D = (np.where(a, left, D) + e[t, :n]).astype(np.float32)
            adv[t] = a
    path = np.zeros(F, dtype=np.int64)
    l = n - 1
    for t in range(F - 1, -1, -1):
        path[t] = l
        if t and adv[t, l]:
            l -= 1
    spans = np.zeros((n, 2), dtype=np.int32)
    for tok in range(n):
        fr = np.nonzero(path == tok)[0]
        spans[tok] = (fr[0], fr[-1] + 1)
    return spans, np.float32(D[n - 1]), path


def viterbi_batch_ref(emit, ntok, nfrm, L):
    """emit float32 [B, T, >= L] -> (spans int32 [B, L, 2], score float32 [B]) with the kernel's
    conventions: (-1, -1) past a pair's tokens; an infeasible pair (n < 1, n > L, F < n, F > T) all
    (-1, -1) and score -inf."""
    emit = np.asarray(emit, dtype=np.float32)
    B, T = emit.shape[:2]
    spans = np.full((B, L, 2), -1, dtype=np.int32)
    score = np.full(B, -np.inf, dtype=np.float32)
    for b in range(B):
        n, F = int(ntok[b]), int(nfrm[b])
        if n < 1 or n > L or F < n or F > T:
            continue
        spans[b, :n], score[b], _ = viterbi_ref(emit[b], n, F)
    return spans, score


def monotone_paths(n, F):
    """Every path l(0) = 0, l(F-1) = n-1, steps in {0, 1}: the frames at which it advances."""
    for cuts in itertools.combinations(range(1, F), n - 1):
        path = np.zeros(F, dtype=np.int64)
        for c in cuts:
            path[c:] += 1
        yield path


def path_score(e, path):
    """The float32 sum of a path's emissions in frame order, as the recurrence adds them."""
    s = np.float32(e[0, path[0]])
    for t in range(1, len(path)):
        s = np.float32(s + np.float32(e[t, path[t]]))
    return s


def planted(L, T, n, F, seed=0, background=-5.0):
    """A [T, L] float32 matrix with zeros on a random monotone path over (n tokens, F frames) and
    `background` elsewhere -> (matrix, spans int32 [n, 2])."""
    rng = np.random.default_rng(seed)
    cuts = np.sort(rng.choice(np.arange(1, F), size=n - 1, replace=False)) if n > 1 else np.zeros(0, dtype=np.int64)
    bounds = np.concatenate([[0], cuts, [F]]).astype(np.int32)
    e = np.full((T, L), background, dtype=np.float32)
    for tok in range(n):
        e[bounds[tok]:bounds[tok + 1], tok] = 0.0
    return e, np.stack([bounds[:-1], bounds[1:]], 1)
