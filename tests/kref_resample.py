"""fp64 numpy restatement of the resampler's definition (include/ste.h "resample").

No bit-level reference exists for this step (the reference resamples through soxr / FFmpeg, whose
filters have no closed form), so the yardstick is the definition itself in double precision: the
coefficient table and a direct per-output dot product.  Nothing here imports the package."""
import math

import numpy as np

ZEROS = 64
ROLLOFF = 0.9475937167399596
BETA = 14.769656459379492


def plan(sr_in, sr_out=16000):
    """(M, L, K, hw, c) of a rate pair."""
    g = math.gcd(sr_in, sr_out)
    M, L = sr_in // g, sr_out // g
    c = ROLLOFF * min(L, M)
    hw = math.ceil(ZEROS * M / c)
    return M, L, 2 * hw, hw, c


def n_out(n_in, M, L):
    return -(-n_in * L // M)


def coeff(num, M, L, c):
    """h at integer numerators num = m·L - n·M (array), in float64."""
    t = np.asarray(num, dtype=np.float64) * c / (M * L)
    inside = np.abs(t) < ZEROS
    ts = np.where(inside, t, 0.0)
    sinc = np.sinc(ts)                                  # sin(pi t)/(pi t), 1 at t = 0
    win = np.i0(BETA * np.sqrt(1.0 - (ts / ZEROS) ** 2)) / np.i0(BETA)
    return np.where(inside, (c / M) * sinc * win, 0.0)


def table(sr_in, sr_out=16000):
    """float64 [K, L]: tap t of phase i (flattened: the tap-major t·L + i of ste_resample_table)."""
    M, L, K, hw, c = plan(sr_in, sr_out)
    i = np.arange(L, dtype=np.int64)
    t = np.arange(K, dtype=np.int64)
    # output n = i: source m = floor(i·M/L) - hw + 1 + t
    m = (i * M // L)[None, :] - hw + 1 + t[:, None]
    return coeff(m * L - i[None, :] * M, M, L, c)


def resample(x, sr_in, sr_out=16000, round_table=False):
    """x float [n_in] -> (y float64 [n_out], bound float64 [n_out] = Σ_m |h·x[m]|), direct dot products.
    round_table: coefficients rounded to fp32 first (what the kernel multiplies by); the default is
    the definition itself, unrounded."""
    M, L, K, hw, c = plan(sr_in, sr_out)
    x = np.asarray(x, dtype=np.float64)
    n_in = x.shape[0]
    N = n_out(n_in, M, L)
    tab = table(sr_in, sr_out)
    if round_table:
        tab = tab.astype(np.float32).astype(np.float64)
    n = np.arange(N, dtype=np.int64)
    base = n * M // L - hw + 1
    xp = np.concatenate([np.zeros(K), x, np.zeros(K + M)])  # zero extension; index m -> m + K
    y = np.zeros(N)
    bound = np.zeros(N)
    ph = n % L
    for t in range(K):
        p = tab[t, ph] * xp[base + t + K]
        y += p
        bound += np.abs(p)
    return y, bound
