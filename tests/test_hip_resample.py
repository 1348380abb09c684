"""gam_op_resample (gam_resample.h) against the fp64 helper tests/resample_ref.py, which tests/test_audio_host.py pins to a second
formulation on the CPU.

Bar: per case max|gpu - fp64| <= K_RS x max(max|ref32 - fp64|, one fp32 ulp of max|y|), ref32 being the same sum
in plain fp32 arithmetic in tap order.  Conversions, downmix, the identity filter, batching and padding are exact: bit-equal."""
import ctypes as C

import numpy as np
import pytest
import torch

from common import report

import gigaam_amd
import resample_ref as R
from gigaam_amd import _lib

pytestmark = pytest.mark.gpu

# K of the bar: twice the largest max|gpu - fp64| / max(max|ref32 - fp64|, ulp) measured on the MI355X, rounded up, at most 8.
# Measured, the largest of every case of this file and of test_hip_audio_e2e.py per rate class: integer decimation
# 1.46 (96 k -> 16 k; 48 k 1.00, 32 k and 16 k -> 8 k 1.09), rational 1.61 (44.1 k -> 16 k; 24 k 1.23, 22.05 k 1.00), upsampling 1.24
# (8 k -> 16 k, the stereo A-law mean; f32 noise 1.13; 11.025 k, 12 k and 1000 -> 1001 1.00).  The kernel's FMA chain rounds once per
# tap where ref32 rounds twice, so ratios below 1 are as common as ratios above.
K_RS = 4

RATE_PAIRS = [(48000, 16000), (8000, 16000), (44100, 16000), (24000, 16000), (22050, 16000), (96000, 16000), (11025, 16000),
              (32000, 16000), (12000, 16000), (16000, 8000),
              (1000, 1001)]          # ... and a table too large for LDS: the tile stages its own rows
# the kernel forms these launch, as (form of gam_resample_tile, upsampling): N = 1; N > 1 with the table in LDS, down and up; rows only
FORMS = {(0, False), (1, False), (1, True), (2, True)}
DEV = "cuda:0"


def lib():
    return _lib.load_library()


def tile_form(rates):
    tile, form = C.c_int(), C.c_int()
    assert lib().gam_resample_tile(rates[0], rates[1], C.byref(tile), C.byref(form)) == 0
    return tile.value, form.value


_TAB = {}


def device_table(rates):
    if rates not in _TAB:
        O, N, K, _ = R.plan(*rates)
        coeff, first = np.empty(N * K, np.float32), np.empty(N, np.int32)
        assert lib().gam_resample_table(rates[0], rates[1], C.c_void_p(coeff.ctypes.data), C.c_void_p(first.ctypes.data)) == 0
        _TAB[rates] = (torch.from_numpy(coeff).to(DEV), torch.from_numpy(first).to(DEV))
    return _TAB[rates]


def op(src, fmt, channels, channel, len_in, B, frames, rates, L_out, want_len=True):
    """One gam_op_resample launch on raw device bytes / samples; (dst [B, L_out] poisoned before the call, len_out)."""
    coeff, first = device_table(rates)
    dst = torch.full((B, L_out), float("nan"), dtype=torch.float32, device=DEV)
    len_out = torch.full((B,), -7, dtype=torch.int64, device=DEV) if want_len else None
    rc = lib().gam_op_resample(C.c_void_p(src.data_ptr()), R.FORMATS.index(fmt), channels, -1 if channel is None else channel,
                               C.c_void_p(0 if len_in is None else len_in.data_ptr()), B, frames, rates[0], rates[1],
                               C.c_void_p(coeff.data_ptr()), C.c_void_p(first.data_ptr()), C.c_void_p(dst.data_ptr()), L_out,
                               C.c_void_p(0 if len_out is None else len_out.data_ptr()),
                               C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, rc
    torch.cuda.synchronize()
    return dst, len_out


def bar_ratio(got, x32, rates, what=None):
    """max|got - fp64| over the bar's denominator, for one signal."""
    ref = R.resample_ref(x32, *rates)
    ref32 = R.resample_ref32(x32, *rates)
    assert got.shape == ref.shape
    den = max(np.abs(ref32 - ref).max(), R.ulp32(np.abs(ref).max()))
    ratio = np.abs(got.astype(np.float64) - ref).max() / den
    if what is not None:
        print(f"resample {rates[0]}->{rates[1]} {what} ratio={ratio:.3f}")
        report("resample_" + what, rates=list(rates), ratio=ratio)
    return ratio


def matrix_sizes(rates):
    """n_in: 1, 2, half a filter, a filter, the first tile boundary - 1 / exact / + 1 in OUTPUT samples, three tiles + 7."""
    O, N, K, _ = R.plan(*rates)
    tile, _ = tile_form(rates)
    sizes = {1, 2, (K + 1) // 2, K}
    for target in (tile - 1, tile, tile + 1, 3 * tile + 7):
        n = max(1, target * O // N)
        while R.out_len(*rates, n) < target:
            n += 1
        sizes.add(n)
    return sorted(sizes), tile


@pytest.mark.parametrize("rates", RATE_PAIRS)
def test_numeric_matrix(rates):
    sizes, tile = matrix_sizes(rates)
    outs = [R.out_len(*rates, n) for n in sizes]
    assert min(outs) < tile < max(outs)
    assert max(outs) >= 3 * tile + 7                                # more than three workgroups per row
    worst = 0.0
    for n in sizes:
        rng = np.random.default_rng(n)
        x = np.stack([rng.standard_normal(n).astype(np.float32), np.where(np.arange(n) % 2 == 0, 1.0, -1.0).astype(np.float32)])
        n_out = R.out_len(*rates, n)
        dst, len_out = op(torch.from_numpy(x).to(DEV), "f32", 1, None, None, 2, n, rates, n_out)
        assert len_out.tolist() == [n_out, n_out]
        got = dst.cpu().numpy()
        for row in range(2):
            ratio = bar_ratio(got[row], x[row], rates)
            print(f"resample {rates[0]}->{rates[1]} n_in={n} n_out={n_out} row={row} ratio={ratio:.3f}")
            worst = max(worst, ratio)
            assert ratio <= K_RS, (rates, n, row, ratio)
    report("resample_matrix", rates=list(rates), worst_ratio=worst, tile=tile)


def test_matrix_covers_every_kernel_form():
    launched = set()
    for rates in RATE_PAIRS:
        O, N, _, _ = R.plan(*rates)
        launched.add((tile_form(rates)[1], N > O))
    assert launched == FORMS, launched ^ FORMS


@pytest.mark.parametrize("rates", [(44100, 16000), (48000, 16000), (8000, 16000), (1000, 1001)])
def test_ragged_batch(rates):
    tile, _ = tile_form(rates)
    O, N, K, _ = R.plan(*rates)
    frames = (2 * tile + 300) * O // N + 5
    lens = [frames, 1, K + 3, (tile + 1) * O // N]
    rng = np.random.default_rng(3)
    x = rng.standard_normal((4, frames)).astype(np.float32)
    padded = x.copy()
    for b, n in enumerate(lens):
        padded[b, n:] = 1e30                                         # the padding of a row counts as zeros whatever it holds
    L_out = R.out_len(*rates, frames) + 9
    dst, len_out = op(torch.from_numpy(padded).to(DEV), "f32", 1, None, torch.tensor(lens, device=DEV), 4, frames, rates, L_out)
    want_len = [R.out_len(*rates, n) for n in lens]
    assert len_out.tolist() == want_len
    for b, n in enumerate(lens):
        alone, _ = op(torch.from_numpy(x[b, :n].copy()).to(DEV), "f32", 1, None, None, 1, n, rates, want_len[b], want_len=False)
        assert torch.equal(dst[b, :want_len[b]], alone[0]), b
        assert bool((dst[b, want_len[b]:] == 0).all()), b            # (the buffer was NaN before the call)
    # len_in = NULL: every row holds `frames`
    dst2, len2 = op(torch.from_numpy(x).to(DEV), "f32", 1, None, None, 4, frames, rates, L_out)
    assert len2.tolist() == [L_out - 9] * 4
    assert torch.equal(dst2[0], dst[0]) and bool((dst2[:, L_out - 9:] == 0).all())
    assert bar_ratio(dst2[3, :L_out - 9].cpu().numpy(), x[3], rates, "ragged") <= K_RS
    # a length beyond the row, and a negative one, are clamped; an output buffer shorter than the result is filled and no further
    short = L_out - 9 - tile - 3
    dst3, len3 = op(torch.from_numpy(x).to(DEV), "f32", 1, None, torch.tensor([frames + 5, -3, frames, 0], device=DEV), 4, frames, rates, short)
    assert len3.tolist() == [short, 0, short, 0]
    assert torch.equal(dst3[0], dst2[0, :short]) and torch.equal(dst3[2], dst2[2, :short]) and bool((dst3[1] == 0).all())


@pytest.mark.parametrize("fmt", R.FORMATS)
def test_formats_at_equal_rates_are_exact(fmt):
    frames = 1031
    for channels in (1, 2, 3, 6):
        raw = R.random_raw(fmt, frames, channels, seed=channels)
        src = torch.from_numpy(raw.copy()).to(DEV)
        x = R.decode_samples(raw, fmt).reshape(frames, channels)
        for channel in sorted({None, 0, channels - 1}, key=lambda c: -1 if c is None else c):
            dst, len_out = op(src, fmt, channels, channel, None, 1, frames, (16000, 16000), frames)
            assert len_out.tolist() == [frames]
            want = R.downmix(x, channel)
            assert np.array_equal(dst[0].cpu().numpy().view(np.uint32), want.view(np.uint32)), (fmt, channels, channel)
    if fmt == "i16":
        assert x.min() == -1.0 and x.max() == np.float32(32767 / 32768)


@pytest.mark.parametrize("fmt,channels,rates", [("alaw", 2, (8000, 16000)), ("i24", 3, (44100, 16000))])
def test_formats_through_the_filter(fmt, channels, rates):
    tile, _ = tile_form(rates)
    O, N, _, _ = R.plan(*rates)
    frames = (tile + 77) * O // N
    lens = [frames, frames // 3]
    raw = np.stack([R.random_raw(fmt, frames, channels, seed=b + 11) for b in range(2)])        # [2, frame bytes]: odd byte strides for i24
    src = torch.from_numpy(raw.copy()).to(DEV)
    for channel in (None, channels - 1):
        dst, len_out = op(src, fmt, channels, channel, torch.tensor(lens, device=DEV), 2, frames, rates, R.out_len(*rates, frames))
        for b, n in enumerate(lens):
            mono = R.decode_ref(raw[b], fmt, channels, channel)[:n]
            n_out = R.out_len(*rates, n)
            assert int(len_out[b]) == n_out
            assert bar_ratio(dst[b, :n_out].cpu().numpy(), mono, rates, f"{fmt}_c{channel}_row{b}") <= K_RS


def test_offsets_beyond_32_bits():
    """u8 mono, 2**31 + 4099 frames, 48 k -> 16 k: the last 4096 outputs against the helper on the last inputs."""
    free, _ = torch.cuda.mem_get_info()
    if free < 8 << 30:
        pytest.skip("needs 8 GB of free device memory")
    rates = (48000, 16000)
    n = 2 ** 31 + 4099
    src = torch.empty(n, dtype=torch.uint8, device=DEV)
    step = 1 << 28
    gen = torch.Generator(device=DEV).manual_seed(5)
    for s in range(0, n, step):
        e = min(n, s + step)
        src[s:e] = torch.randint(0, 256, (e - s,), dtype=torch.uint8, device=DEV, generator=gen)
    n_out = R.out_len(*rates, n)
    assert n_out > 2 ** 29
    dst, len_out = op(src, "u8", 1, None, None, 1, n, rates, n_out)
    assert len_out.tolist() == [n_out]
    tail_in = 3 * (4096 + 64) + n % 3                               # starts on a multiple of O = 3: output phases line up
    start = n - tail_in
    assert start % 3 == 0 and start > 2 ** 31 - 3 * 4200
    mono = R.decode_samples(src[start:].cpu().numpy(), "u8")
    ref, ref32 = R.resample_ref(mono, *rates)[-4096:], R.resample_ref32(mono, *rates)[-4096:]
    got = dst[0, -4096:].cpu().numpy()
    assert start // 3 + R.out_len(*rates, tail_in) == n_out
    den = max(np.abs(ref32 - ref).max(), R.ulp32(np.abs(ref).max()))
    ratio = np.abs(got - ref).max() / den
    print(f"resample 48000->16000 tail of 2**31 + 4099 ratio={ratio:.3f}")
    assert ratio <= K_RS
    # ... and an early stretch, so that a wrapped index cannot have written the right values in the wrong place only
    head = R.decode_samples(src[:3 * 5000].cpu().numpy(), "u8")
    assert np.abs(dst[0, :4096].cpu().numpy() - R.resample_ref(head, *rates)[:4096]).max() / den <= K_RS
    del src, dst


@pytest.mark.parametrize("rate", [48000, 44100, 8000])
def test_a_sine_keeps_its_amplitude(rate):
    n = rate // 4
    x = torch.sin(2 * torch.pi * 1000.0 * torch.arange(n, dtype=torch.float64) / rate).float().to(DEV)
    y = gigaam_amd.resample(x, rate, 16000)
    assert y.shape == (R.out_len(rate, 16000, n),)
    y = y.double().cpu().numpy()[400:-400]                             # away from the ends, where the filter sees the zeros outside
    ph = 2 * np.pi * 1000.0 * np.arange(400, 400 + y.shape[0]) / 16000.0
    basis = np.stack([np.sin(ph), np.cos(ph)], 1)
    a, b = np.linalg.lstsq(basis, y, rcond=None)[0]
    assert abs(np.hypot(a, b) - 1.0) < 2e-3
