"""ORACLE (test infrastructure only — never imported by the product path).

numpy replica of the dropout generator of the HIP kernels (csrc/ldetr_common.hpp: rng_bits, drop_scale): a pure function of (seed, element
index), so every mask a kernel draws can be rebuilt on the host and an fp64 reference that multiplies by it is a full reference for train mode.

  seed   the 64-bit sum (mod 2^64) of the host half (hip.core.next_seed(), one draw per launch with p > 0) and the device half (the word
         hip.core.iter_seed() holds): total_seed
  index  one convention per site, shared by the forward kernel and its backward:
           attention probabilities   ((b*H + h)*Lq + q)*Lk + key      attention_index / attention_scale  -> [B, H, Lq, Lk]
           LayerNorm residual        row*D + col                      rows_index / layernorm_scale       -> [rows, D]
           feed-forward hidden       m*F + col                        rows_index / hidden_scale          -> [M, F]
           GEMM epilogue             row*ldc + col                    rows_index / gemm_scale            -> [rows, cols]
  keep   u = float32(bits >> 8) * 2^-24 >= float32(p); a kept element is scaled by 1 / (1 - float32(p)), a dropped one is 0.

Pinned by tests/test_dropout_ref_cpu.py against vectors computed from a C transcription of the header.
"""
import numpy as np

_M64 = (1 << 64) - 1


def total_seed(host_seed, device_word):
    """(host half + device half) mod 2^64, as the kernels add them; the device word may be given as the signed int64 that .item() returns."""
    return (int(host_seed) + int(device_word)) & _M64


def rng_bits(seed, idx):
    """uint32 bits of element `idx` (uint64 array) under `seed` (Python int, taken mod 2^64)."""
    seed = int(seed) & _M64
    idx = np.atleast_1d(np.asarray(idx, dtype=np.uint64))
    s_lo, s_hi = np.uint32(seed & 0xFFFFFFFF), np.uint32(seed >> 32)
    with np.errstate(over='ignore'):
        x = (idx & np.uint64(0xFFFFFFFF)).astype(np.uint32) ^ s_lo
        x = x * np.uint32(0xcc9e2d51)
        x = (x << np.uint32(15)) | (x >> np.uint32(17))
        x = x ^ (s_hi + (idx >> np.uint64(32)).astype(np.uint32) * np.uint32(0x1b873593))
        x = x ^ (x >> np.uint32(16)); x = x * np.uint32(0x85ebca6b)
        x = x ^ (x >> np.uint32(13)); x = x * np.uint32(0xc2b2ae35)
        x = x ^ (x >> np.uint32(16))
    return x.astype(np.uint32)


def keep(seed, idx, p):
    """bool array: element idx survives dropout with probability-of-dropping p (rounded to float32, as the C ABI passes it)."""
    u = (rng_bits(seed, idx) >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)
    return u >= np.float32(p)


def keep_scale(p):
    """What a kept element is multiplied by."""
    return 1.0 / (1.0 - float(np.float32(p)))


def scale(seed, idx, p):
    """float64 array shaped like idx: 0 where dropped, 1 / (1 - p) where kept."""
    idx = np.asarray(idx, dtype=np.uint64)
    return (keep(seed, idx.reshape(-1), p).astype(np.float64) * keep_scale(p)).reshape(idx.shape)


def attention_index(B, H, Lq, Lk):
    """[B, H, Lq, Lk] uint64: ((b*H + h)*Lq + q)*Lk + key."""
    bh = np.arange(B * H, dtype=np.uint64).reshape(B, H, 1, 1)
    q = np.arange(Lq, dtype=np.uint64).reshape(1, 1, Lq, 1)
    k = np.arange(Lk, dtype=np.uint64).reshape(1, 1, 1, Lk)
    return (bh * np.uint64(Lq) + q) * np.uint64(Lk) + k


def rows_index(rows, cols, ld=None):
    """[rows, cols] uint64: row*ld + col (ld: the row pitch the kernel indexes with; default cols)."""
    ld = cols if ld is None else ld
    return np.arange(rows, dtype=np.uint64).reshape(rows, 1) * np.uint64(ld) + np.arange(cols, dtype=np.uint64).reshape(1, cols)


def attention_scale(seed, p, B, H, Lq, Lk):
    """[B, H, Lq, Lk]: what the probabilities of (batch b, head h, query q, key) are multiplied by."""
    return scale(seed, attention_index(B, H, Lq, Lk), p)


def layernorm_scale(seed, p, rows, D):
    """[rows, D]: what the residual branch r of LayerNorm(x + dropout(r)) is multiplied by."""
    return scale(seed, rows_index(rows, D), p)


def hidden_scale(seed, p, M, F):
    """[M, F]: what the hidden activation (after the relu) of the fused feed-forward launch is multiplied by."""
    return scale(seed, rows_index(M, F), p)


def gemm_scale(seed, p, rows, cols, ldc=None):
    """[rows, cols]: what the GEMM epilogue multiplies its output by (after bias and activation); ldc: the output's row pitch."""
    return scale(seed, rows_index(rows, cols, ldc), p)
