"""Reference for the free-endpoint decode (ste_align_spot) in numpy float32, with exactly
the recurrence, the two strict tie rules and the walk back of include/ste.h.  tests/test_spot_cpu.py
pins it to a brute-force enumeration of every (start, end, monotone path)."""
import itertools

import numpy as np


def spot_ref(e, m, F, bg, lead=0):
    """One pair.  e float32 [T, >= lead + m] frame-major emissions, m phrase tokens in columns
    lead .. lead+m-1, F frames, bg the background per frame ->
    (spans int32 [m, 2] as (first frame, last frame + 1), hit (start, end), score float32), or None when
    no D_t[m-1] exceeds -inf.
    g = e - bg (one float32 subtract); from D_{-1} = -inf: left_0 = +0, left_j = D_{t-1}[j-1];
    adv = left > D_{t-1} (strict); D_t = (adv ? left : D_{t-1}) + g[t] (one float32 add); the end is
    the earliest t that attains max_t D_t[m-1]; the walk back starts at (t_best, m-1)."""
    e = np.asarray(e, dtype=np.float32)
    assert 1 <= m <= e.shape[1] - lead and m <= F <= e.shape[0]
    bg = np.float32(bg)
    D = np.full(m, -np.inf, dtype=np.float32)
    adv = np.zeros((F, m), dtype=bool)
    best, t_best = np.float32(-np.inf), -1
    with np.errstate(invalid="ignore", over="ignore"):
        for t in range(F):
            g = (e[t, lead:lead + m] - bg).astype(np.float32)
            left = np.concatenate([np.float32([0.0]), D[:-1]])
            a = left > D
            D = (np.where(a, left, D) + g).astype(np.float32)
            adv[t] = a
            if D[m - 1] > best:
                best, t_best = np.float32(D[m - 1]), t
    if t_best < 0:
        return None
    start = np.zeros(m + 1, dtype=np.int32)
    start[m] = t_best + 1
    t, j = t_best, m - 1
    while t >= 0:
        start[j] = t
        if adv[t, j]:
            j -= 1
            if j < 0:
                break
        t -= 1
    spans = np.stack([start[:-1], start[1:]], 1).astype(np.int32)
    return spans, (int(start[0]), t_best + 1), best


def spot_batch_ref(emit, ntok, nfrm, bg, lead, L):
    """emit float32 [B, T, >= L] -> (spans int32 [B, L, 2], hit int32 [B, 2], score float32 [B]) with the
    kernel's conventions: (-1, -1) on every row outside lead .. lead+m-1; an infeasible pair (m < 1,
    lead + m > L, F < m, F > T) all (-1, -1) and score -inf."""
    emit = np.asarray(emit, dtype=np.float32)
    B, T = emit.shape[:2]
    spans = np.full((B, L, 2), -1, dtype=np.int32)
    hit = np.full((B, 2), -1, dtype=np.int32)
    score = np.full(B, -np.inf, dtype=np.float32)
    for b in range(B):
        m, F = int(ntok[b]), int(nfrm[b])
        if m < 1 or lead + m > L or F < m or F > T:
            continue
        r = spot_ref(emit[b], m, F, bg[b], lead)
        if r is not None:
            spans[b, lead:lead + m], hit[b], score[b] = r
    return spans, hit, score


def spot_paths(m, F):
    """Every hit: (start, end, bounds int [m + 1]) with start = bounds[0] < bounds[1] < ... < bounds[m] =
    end <= F; token j holds frames bounds[j] .. bounds[j+1] - 1."""
    for bounds in itertools.combinations(range(F + 1), m + 1):
        yield bounds[0], bounds[-1], np.asarray(bounds)


def gain_sum(e, bounds, bg, lead=0):
    """The float32 sum of a hit's gains in frame order, as the recurrence adds them (from +0)."""
    s = np.float32(0.0)
    for j in range(len(bounds) - 1):
        for t in range(bounds[j], bounds[j + 1]):
            s = np.float32(s + np.float32(np.float32(e[t, lead + j]) - np.float32(bg)))
    return s
