"""Audio ingest at recording size: one hour of 48 kHz stereo PCM16 (691 MB) and one hour of 8 kHz A-law (29 MB), to mono fp32 at 16 kHz.
Times (a) gam_op_resample alone, by device events around launches on bytes already on the device, (b) ``decode_audio`` end to end --
file read (page cache warm: the file was just written), upload and kernel, a host clock around a call that ends in a device
synchronise -- and (c) ``load_audio(backend="ffmpeg")`` on the same files where ffmpeg is installed.  The kernel's rate is quoted over
the bytes the algorithm needs (raw input + fp32 output).  A tool, not a test: no threshold; one JSON line per measurement.

    python tools/audio_ingest_bench.py [--seconds 3600] [--repeat 5] [--dir DIR]"""
import argparse
import ctypes as C
import json
import os
import shutil
import statistics
import struct
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import gigaam_amd  # noqa: E402
from gigaam_amd import _lib, audio  # noqa: E402


def write_wav(path, tag, channels, rate, bits, seconds, rng):
    """A WAV of `seconds` of noise: one minute of random samples, repeated (the kernel's work does not depend on the values)."""
    block = channels * bits // 8
    total = seconds * rate * block
    minute = min(total, 60 * rate * block)
    if bits == 16:
        chunk = rng.integers(-20000, 20000, minute // 2).astype("<i2").tobytes()
    else:
        chunk = rng.integers(0, 256, minute, dtype=np.uint8).tobytes()
    fmt = struct.pack("<HHIIHH", tag, channels, rate, rate * block, block, bits)
    with open(path, "wb") as fh:
        fh.write(b"RIFF" + struct.pack("<I", 4 + 8 + len(fmt) + 8 + total) + b"WAVE" + b"fmt " + struct.pack("<I", len(fmt)) + fmt)
        fh.write(b"data" + struct.pack("<I", total))
        left = total
        while left > 0:
            fh.write(chunk[:left])
            left -= min(left, len(chunk))


def time_kernel(wav, dev, repeat):
    """Median / min milliseconds of gam_op_resample alone on the file's bytes."""
    src = torch.from_numpy(wav.data).to(dev)
    n_out = audio._out_len(wav.rate, 16000, wav.frames)
    for _ in range(2):                                   # warm-up: code object load, table upload
        audio._run(src, wav.fmt, wav.channels, None, None, 1, wav.frames, wav.rate, 16000, n_out, False)
    torch.cuda.synchronize(dev)
    ms = []
    for _ in range(repeat):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        audio._run(src, wav.fmt, wav.channels, None, None, 1, wav.frames, wav.rate, 16000, n_out, False)
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms), min(ms), wav.data.size + 4 * n_out


def time_call(fn, repeat):
    out = []
    for _ in range(repeat):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append(time.perf_counter() - t0)
    return statistics.median(out), min(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=int, default=3600)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--dir", default=None, help="where the generated files go (default: the system's temporary directory)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise _lib.GigaAMHipError("audio_ingest_bench needs the GPU: a CPU run measures nothing")
    dev = torch.device("cuda", 0)
    have_ffmpeg = shutil.which("ffmpeg") is not None
    rng = np.random.default_rng(0)
    with tempfile.TemporaryDirectory(dir=args.dir) as d:
        for name, tag, channels, rate, bits in (("48k_stereo_pcm16", 1, 2, 48000, 16), ("8k_alaw", 6, 1, 8000, 8)):
            path = os.path.join(d, name + ".wav")
            write_wav(path, tag, channels, rate, bits, args.seconds, rng)
            wav = gigaam_amd.read_wav(path)
            med, lo, nbytes = time_kernel(wav, dev, args.repeat)
            print(json.dumps({"input": name, "what": "gam_op_resample alone", "audio_s": args.seconds, "ms_median": round(med, 4), "ms_min": round(lo, 4),
                              "algorithmic_bytes": nbytes, "GB_per_s": round(nbytes / med / 1e6, 1), "x_realtime": round(args.seconds / (med / 1e3))}), flush=True)
            del wav
            gigaam_amd.decode_audio(path, device=dev)                              # warm-up
            med, lo = time_call(lambda: gigaam_amd.decode_audio(path, device=dev), args.repeat)
            print(json.dumps({"input": name, "what": "decode_audio end to end (read + H2D + kernel)", "audio_s": args.seconds, "s_median": round(med, 4),
                              "s_min": round(lo, 4), "x_realtime": round(args.seconds / med)}), flush=True)
            if have_ffmpeg:
                med, lo = time_call(lambda: gigaam_amd.load_audio(path, backend="ffmpeg"), max(1, args.repeat // 2))
                print(json.dumps({"input": name, "what": "load_audio(backend='ffmpeg')", "audio_s": args.seconds, "s_median": round(med, 4),
                                  "s_min": round(lo, 4), "x_realtime": round(args.seconds / med)}), flush=True)
            else:
                print(json.dumps({"input": name, "what": "load_audio(backend='ffmpeg')", "result": "not measured: no ffmpeg"}), flush=True)
            os.unlink(path)


if __name__ == "__main__":
    main()
