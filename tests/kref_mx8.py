"""What stored MX-fp8 bytes mean, restated in numpy from the raw bytes (no op of the library):

    value = bf16( float(e4m3 byte) · 2^(E − 127) )        E the block's E8M0 byte, one per 32 columns

OCP e4m3: 1 sign, 4 exponent (bias 7), 3 mantissa bits; exponent 0 is subnormal (m/8 · 2^-6, the
smallest 2^-9); no infinities; S.1111.111 is NaN; the largest finite value is 1.75 · 2^8 = 448.
E8M0: 2^(E − 127), E = 255 is NaN.  The product is formed in float32: it has 4 significant bits and is
at least 2^-136, so it is exact there (subnormals kept) unless it reaches 2^128 (E >= 247 only), where
it is ±inf.  bf16 keeps 8 significant bits over float32's exponent range, so the final rounding (to
nearest even) changes a value only below 2^-126, in bf16's subnormal range.
"""
import numpy as np


def e4m3_to_float64(b):
    """uint8 array of OCP e4m3 bytes -> float64 (NaN for 0x7f / 0xff)."""
    b = np.asarray(b, dtype=np.uint8).astype(np.int64)
    sign = np.where(b >> 7 == 1, -1.0, 1.0)
    ex, man = (b >> 3) & 15, b & 7
    mag = np.where(ex == 0, np.ldexp(man / 8.0, -6), np.ldexp(1.0 + man / 8.0, ex - 7))
    return np.where((ex == 15) & (man == 7), np.nan, sign * mag)


def e8m0_to_float64(e):
    """uint8 array of E8M0 scale bytes -> float64 2^(E − 127) (NaN for 0xff)."""
    e = np.asarray(e, dtype=np.uint8).astype(np.int64)
    return np.where(e == 255, np.nan, np.ldexp(1.0, e - 127))


def bf16_bits(x):
    """float64 array (each value exact in float32) -> uint16 bf16 bits, round to nearest even; NaN -> 0x7fc0."""
    x = np.asarray(x, dtype=np.float64)
    with np.errstate(over="ignore"):
        f = x.astype(np.float32)                     # a product of 2^128 or more is ±inf, as in fp32 arithmetic
    fits = np.abs(x) < 2.0 ** 128
    assert np.array_equal(f.astype(np.float64)[fits], x[fits]), "not exact in fp32"
    u = f.view(np.uint32).astype(np.uint64)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)
    return np.where(np.isnan(f), np.uint16(0x7FC0), r)


def bf16_bits_to_float64(bits):
    return (np.asarray(bits, dtype=np.uint16).astype(np.uint32) << 16).view(np.float32).astype(np.float64)


def mx8_dequant_bits(q, scales):
    """q uint8 [rows, K], scales uint8 [rows, K/32] -> bf16 bits uint16 [rows, K]."""
    q, scales = np.asarray(q, dtype=np.uint8), np.asarray(scales, dtype=np.uint8)
    rows, K = q.shape
    assert K % 32 == 0 and scales.shape == (rows, K // 32)
    with np.errstate(invalid="ignore"):
        return bf16_bits(e4m3_to_float64(q) * np.repeat(e8m0_to_float64(scales), 32, axis=1))


def mx8_dequant(q, scales):
    """The same as float64 values."""
    return bf16_bits_to_float64(mx8_dequant_bits(q, scales))


def same_bf16(bits_a, bits_b):
    """Bit equality of two bf16 bit arrays, any NaN equal to any NaN."""
    a, b = np.asarray(bits_a, dtype=np.uint16), np.asarray(bits_b, dtype=np.uint16)
    na, nb = (a & 0x7FFF) > 0x7F80, (b & 0x7FFF) > 0x7F80
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(a[~na], b[~nb])
