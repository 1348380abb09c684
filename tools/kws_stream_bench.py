"""Keyword search over a whole recording (gam_op_ctc_kws_stream): what the resumable search costs at one hour.
(a) ``op_ctc_kws_stream`` alone on synthetic log-probs [90 000, 34] for K = 10 / 100 / 1000 keywords, as ONE call and as calls of one
window batch's rows (16 windows x 334 kept frames), by device events around the launches, the two variants interleaved; (b) on
``workloads.config5_audio``, ``find_keywords_longform(vad="windows")`` with the search on the decode side stream (the default) and on the launch stream
(GAM_KWS_STREAM_OVERLAP=0), against ``transcribe_longform(vad="windows")`` of the same file in the same session -- the encode + stitch
the two share --, a host clock around calls that end in a device-to-host copy, the three interleaved.  What counts is the search's ADDED
wall time over that baseline.  A tool, not a test: no threshold; one JSON line per measurement.

    python tools/kws_stream_bench.py [--seconds 3600] [--repeat 5] [--layers 16] [--dir DIR]"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time
import wave

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import gigaam_amd  # noqa: E402
from gigaam_amd import _lib, synth, workloads  # noqa: E402
from gigaam_amd.decoding import keyword_min_scores  # noqa: E402

T_HOUR, V, BATCH_ROWS = 90000, 34, 16 * 334


def keywords(rng, k, v):
    return [[int(c) for c in rng.integers(0, v - 1, int(rng.integers(3, 9)))] for _ in range(k)]


def time_op(eng, lp, pieces, repeat):
    """{piece: (median, min) milliseconds} of one stream over ``lp`` in calls of ``piece`` rows, BEGIN .. END, for each piece size of
    ``pieces``: device events around the launches, the variants INTERLEAVED (every round runs each once, in turn).  The stream object
    (its state and hit buffers: two allocations and a fill) is made outside the events; inside them are the row-maximum and search
    launches of every push, the END call and ``finish``'s one-word fill of the flag."""
    def run(piece, timed):
        s = eng.kws_stream(8)
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for r in range(0, lp.shape[0], piece):
            s.push(lp[r:r + piece])
        s.finish()
        b.record()
        b.synchronize()
        if timed:
            ms[piece].append(a.elapsed_time(b))
    ms = {piece: [] for piece in pieces}
    for r in range(repeat + 1):                               # (round 0 warms up and is dropped)
        for piece in pieces:
            run(piece, r > 0)
    return {piece: (statistics.median(v), min(v)) for piece, v in ms.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=int, default=3600)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--layers", type=int, default=16)
    ap.add_argument("--dir", default=None, help="where the generated file goes (default: the system's temporary directory)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise _lib.GigaAMHipError("kws_stream_bench needs the GPU: a CPU run measures nothing")
    rng = np.random.default_rng(0)
    model = gigaam_amd.model_from_checkpoint(synth.make_checkpoint("v2_ctc", seed=1, n_layers=args.layers), "cuda:0")
    eng = model.head.engine

    # (a) the search alone
    x = rng.standard_normal((T_HOUR, V)).astype(np.float32)
    np.put_along_axis(x, np.where(rng.random(T_HOUR) < 0.6, V - 1, rng.integers(0, V, T_HOUR))[:, None], 9.0, axis=1)
    lp = torch.log_softmax(torch.from_numpy(x), dim=-1).to("cuda:0")
    for k in (10, 100, 1000):
        kws = keywords(rng, k, V)
        eng.set_keywords(kws, keyword_min_scores([len(y) for y in kws], 0.5))
        variants = {T_HOUR: "one call", BATCH_ROWS: f"calls of {BATCH_ROWS} rows"}
        for piece, (med, lo) in time_op(eng, lp, list(variants), args.repeat).items():
            print(json.dumps({"what": "op_ctc_kws_stream alone, " + variants[piece], "frames": T_HOUR, "V": V, "K": k, "ms_median": round(med, 3),
                              "ms_min": round(lo, 3), "us_per_frame": round(med * 1e3 / T_HOUR, 4)}), flush=True)
    del lp

    # (b) the model call against the encode + stitch it shares with transcribe_longform(vad="windows")
    audio = workloads.config5_audio(args.seconds)
    vocab = len(model.decoding.tokenizer)
    kws = keywords(rng, 10, vocab + 1)
    calls = {
        "transcribe_longform(vad='windows') [shared encode + stitch]": (None, lambda p: model.transcribe_longform(p, vad="windows")),
        "find_keywords_longform(vad='windows'), overlap on": ("1", lambda p: model.find_keywords_longform(p, kws, vad="windows")),
        "find_keywords_longform(vad='windows'), overlap off": ("0", lambda p: model.find_keywords_longform(p, kws, vad="windows")),
    }
    with tempfile.TemporaryDirectory(dir=args.dir) as d:
        path = os.path.join(d, "hour.wav")
        with wave.open(path, "wb") as wf:
            wf.setnchannels(1)
            wf.setsampwidth(2)
            wf.setframerate(16000)
            wf.writeframes((audio.numpy() * 32768.0).round().clip(-32768, 32767).astype(np.int16).tobytes())
        del audio
        times = {name: [] for name in calls}
        for r in range(args.repeat + 1):                      # (round 0 warms every shape up and is dropped)
            for name, (env, fn) in calls.items():             # interleaved: each round runs the three once
                if env is not None:
                    os.environ["GAM_KWS_STREAM_OVERLAP"] = env
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                out = fn(path)
                torch.cuda.synchronize()
                if r:
                    times[name].append(time.perf_counter() - t0)
                os.environ.pop("GAM_KWS_STREAM_OVERLAP", None)
        base = None
        for name, ts in times.items():
            med = statistics.median(ts)
            base = med if base is None else base
            print(json.dumps({"what": name, "audio_s": args.seconds, "layers": args.layers, "K": len(kws), "s_median": round(med, 4),
                              "s_min": round(min(ts), 4), "s_max": round(max(ts), 4), "added_ms_over_shared": round((med - base) * 1e3, 2)}),
                  flush=True)
        del out


if __name__ == "__main__":
    main()
