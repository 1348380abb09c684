"""fp64 numpy statement of the audio-ingest contract (include/gigaam_hip.h, "audio ingest"), written from the formulas and independent of
the library: the resampling plan and table, the filter in fp64 and in the kernel's fp32 arithmetic, the sample-format decoders and the
downmix.  No audioop (gone in Python 3.13), no torchaudio.

With g = gcd(r_in, r_out), O = r_in / g, N = r_out / g, f = 0.99 min(O, N), L = 6 and x[m] = 0 outside [0, n_in):
    y[j] = (f / O) sum_m x[m] sinc(pi t) cos^2(pi t / (2 L)),   t = f (m / O - j / N),   over the m with |t| < L,   j < ceil(N n_in / O).
"""
import math
from fractions import Fraction

import numpy as np

WIDTH = 6
ROLLOFF = Fraction(99, 100)
FORMATS = ["u8", "i16", "i24", "i32", "f32", "mulaw", "alaw"]      # the kernel's format codes, in order
BYTES = {"u8": 1, "i16": 2, "i24": 3, "i32": 4, "f32": 4, "mulaw": 1, "alaw": 1}

_PLANS = {}


def plan(r_in, r_out):
    """(O, N, K, first [N] int64): the support of phase p is the integers m with |f (m / O - p / N)| < L, in exact arithmetic; equal
    rates are the identity."""
    key = (r_in, r_out)
    if key not in _PLANS:
        if r_in == r_out:
            _PLANS[key] = (1, 1, 1, np.zeros(1, np.int64))
        else:
            g = math.gcd(r_in, r_out)
            O, N = r_in // g, r_out // g
            c = Fraction(WIDTH * O) / (ROLLOFF * min(O, N))
            first, K = [], 0
            for p in range(N):
                lo = math.floor(Fraction(p * O, N) - c) + 1            # smallest integer above the open interval's lower end
                hi = math.ceil(Fraction(p * O, N) + c) - 1
                first.append(lo)
                K = max(K, hi - lo + 1)
            _PLANS[key] = (O, N, K, np.array(first, np.int64))
    return _PLANS[key]


_TABLES = {}


def table(r_in, r_out):
    """coeff fp64 [N, K] (zeros beyond a row's support), first int64 [N]."""
    key = (r_in, r_out)
    if key not in _TABLES:
        O, N, K, first = plan(r_in, r_out)
        if r_in == r_out:
            _TABLES[key] = (np.ones((1, 1)), first)
        else:
            f = 0.99 * min(O, N)
            m = first[:, None] + np.arange(K)[None, :]
            t = f * (m * N - np.arange(N)[:, None] * O).astype(np.float64) / float(O * N)
            safe = np.where(t == 0.0, 1.0, t)
            sinc = np.where(t == 0.0, 1.0, np.sin(np.pi * safe) / (np.pi * safe))
            c = (f / O) * sinc * np.cos(np.pi * t / (2.0 * WIDTH)) ** 2
            _TABLES[key] = (np.where(np.abs(t) < WIDTH, c, 0.0), first)
    return _TABLES[key]


def out_len(r_in, r_out, n_in):
    O, N, _, _ = plan(r_in, r_out)
    return -((-N * int(n_in)) // O)


def _gather(x, r_in, r_out, dtype):
    """The taps of every output, [n_out, K], and their coefficients [n_out, K]."""
    O, N, K, first = plan(r_in, r_out)
    coeff, _ = table(r_in, r_out)
    n_in = x.shape[0]
    n_out = out_len(r_in, r_out, n_in)
    j = np.arange(n_out, dtype=np.int64)
    m = (first[j % N] + (j // N) * O)[:, None] + np.arange(K)[None, :]
    ok = (m >= 0) & (m < n_in)
    taps = np.where(ok, x.astype(dtype)[np.clip(m, 0, max(n_in - 1, 0))] if n_in else 0, 0).astype(dtype)
    return taps, coeff.astype(dtype)[j % N]


def resample_ref(x, r_in, r_out):
    """fp64."""
    taps, c = _gather(np.asarray(x, np.float64), r_in, r_out, np.float64)
    return (taps * c).sum(1)


def resample_ref32(x, r_in, r_out):
    """The same sum as plain fp32 arithmetic: fp32 coefficients, products and additions rounded to fp32, in tap order."""
    taps, c = _gather(np.asarray(x, np.float32), r_in, r_out, np.float32)
    acc = taps[:, 0] * c[:, 0]
    for k in range(1, taps.shape[1]):
        acc = (acc + taps[:, k] * c[:, k]).astype(np.float32)
    return acc


def ulp32(v):
    return 2.0 ** (math.floor(math.log2(v)) - 23) if v > 0 else 2.0 ** -149


# ------------------------------------------------------------------------------------------------------------ formats
def mulaw_decode(b):
    u = (~np.asarray(b, np.uint8)).astype(np.int32) & 0xFF
    mag = ((((u & 15) << 3) + 0x84) << ((u >> 4) & 7)) - 0x84
    return np.where(u & 0x80, -mag, mag).astype(np.int32)


def alaw_decode(b):
    a = (np.asarray(b, np.uint8).astype(np.int32) ^ 0x55) & 0xFF
    e, m = (a >> 4) & 7, a & 15
    mag = np.where(e > 0, ((m << 4) + 0x108) << np.maximum(e - 1, 0), (m << 4) + 8)
    return np.where(a & 0x80, mag, -mag).astype(np.int32)


def decode_samples(raw, fmt):
    """raw: uint8 bytes of interleaved samples -> fp32 [samples]."""
    raw = np.ascontiguousarray(raw, np.uint8).reshape(-1)
    if fmt == "u8":
        return ((raw.astype(np.int32) - 128).astype(np.float32) / np.float32(128.0)).astype(np.float32)
    if fmt == "i16":
        return (raw.view("<i2").astype(np.float32) / np.float32(32768.0)).astype(np.float32)
    if fmt == "i24":
        b = raw.reshape(-1, 3).astype(np.int32)
        v = b[:, 0] | (b[:, 1] << 8) | (b[:, 2] << 16)
        v = np.where(v >= 1 << 23, v - (1 << 24), v)
        return (v.astype(np.float32) / np.float32(8388608.0)).astype(np.float32)
    if fmt == "i32":
        return (raw.view("<i4").astype(np.float32) * np.float32(2.0 ** -31)).astype(np.float32)
    if fmt == "f32":
        return raw.view("<f4").copy()
    if fmt == "mulaw":
        return (mulaw_decode(raw).astype(np.float32) / np.float32(32768.0)).astype(np.float32)
    if fmt == "alaw":
        return (alaw_decode(raw).astype(np.float32) / np.float32(32768.0)).astype(np.float32)
    raise ValueError(fmt)


def downmix(x, channel=None):
    """x fp32 [frames, C] -> fp32 [frames]: channel k, or the mean as an fp32 sum in channel order times fp32(1 / C)."""
    x = np.asarray(x, np.float32)
    if channel is not None:
        return x[:, channel].copy()
    s = x[:, 0].copy()
    for c in range(1, x.shape[1]):
        s = (s + x[:, c]).astype(np.float32)
    return (s * (np.float32(1.0) / np.float32(x.shape[1]))).astype(np.float32)


def decode_ref(raw, fmt, channels, channel=None):
    return downmix(decode_samples(raw, fmt).reshape(-1, channels), channel)


def random_raw(fmt, frames, channels, seed):
    """Raw bytes of `frames` interleaved frames in format fmt (uint8 array), values over the whole range."""
    rng = np.random.default_rng(seed)
    n = frames * channels
    if fmt in ("u8", "mulaw", "alaw"):
        return rng.integers(0, 256, n, dtype=np.uint8)
    if fmt == "i16":
        v = rng.integers(-32768, 32768, n).astype("<i2")
        v[:2] = [-32768, 32767][:min(2, n)]
        return v.view(np.uint8)
    if fmt == "i24":
        v = rng.integers(-(1 << 23), 1 << 23, n).astype(np.int64)
        v[:2] = [-(1 << 23), (1 << 23) - 1][:min(2, n)]
        u = (v & 0xFFFFFF).astype(np.uint32)
        return np.stack([u & 255, (u >> 8) & 255, (u >> 16) & 255], 1).astype(np.uint8).reshape(-1)
    if fmt == "i32":
        v = rng.integers(-(1 << 31), 1 << 31, n).astype("<i4")
        v[:2] = [-(1 << 31), (1 << 31) - 1][:min(2, n)]
        return v.view(np.uint8)
    if fmt == "f32":
        return rng.standard_normal(n).astype("<f4").view(np.uint8)
    raise ValueError(fmt)
