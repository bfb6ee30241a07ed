"""Reference for the retrieval tests: float64 scores on the CPU, ordered by value descending
then index ascending (np.lexsort((index, -S))).  brute_force_topk applies the order's definition
pair by pair; test_retrieval_cpu.py checks the two against each other under ties."""
import numpy as np


def scores64(q, corpus):
    return np.asarray(q, dtype=np.float64) @ np.asarray(corpus, dtype=np.float64).T


def lexsort_topk(S, k, base=0):
    """(values float64 [Q, k], indices int64 [Q, k]); the tail beyond N is (-inf, -1)."""
    Q, N = S.shape
    v = np.full((Q, k), -np.inf)
    i = np.full((Q, k), -1, dtype=np.int64)
    idx = np.arange(N)
    for r in range(Q):
        order = np.lexsort((idx, -S[r]))[:k]
        v[r, :len(order)] = S[r, order]
        i[r, :len(order)] = order + base
    return v, i


def brute_force_topk(S, k, base=0):
    Q, N = S.shape
    v = np.full((Q, k), -np.inf)
    i = np.full((Q, k), -1, dtype=np.int64)
    for r in range(Q):
        left = list(range(N))
        for e in range(min(k, N)):
            best = left[0]
            for j in left[1:]:
                if S[r, j] > S[r, best] or (S[r, j] == S[r, best] and j < best):
                    best = j
            left.remove(best)
            v[r, e], i[r, e] = S[r, best], best + base
    return v, i


def ref_ranks(S, targets):
    """Position of targets[r] (an index into S's columns, -1 = none) in row r's lexsorted order."""
    Q, N = S.shape
    idx = np.arange(N)
    out = np.full(Q, -1, dtype=np.int64)
    for r, t in enumerate(np.asarray(targets)):
        if t >= 0:
            out[r] = int(np.nonzero(np.lexsort((idx, -S[r])) == t)[0][0])
    return out
