"""CTC beam search over a whole recording (gam_op_ctc_beam_stream): what the resumable search costs at one hour.
(a) ``op_ctc_beam_stream`` alone on synthetic peaked log-probs [90 000, 34] for W = 4 / 8 / 32, as ONE call and as calls of one window
batch's rows (16 windows x 334 kept frames: 17 calls), by device events around the launches, the two variants interleaved; the END
call (final pick and backtrack: one dependent load per token) is timed by events of its own; (b) on ``workloads.config5_audio``,
``transcribe_longform(vad="windows", stream_search=True, beam_size=8)`` with the search on the decode side stream (the default) and on
the launch stream (GAM_BEAM_STREAM_OVERLAP=0), against the greedy ``transcribe_longform(vad="windows")`` of the same file in the same
session -- the encode + stitch they share --, a host clock around calls that end in a device-to-host copy, the three interleaved.  A
tool, not a test: no threshold; one JSON line per measurement.

    python tools/beam_stream_bench.py [--seconds 3600] [--repeat 9] [--layers 16] [--dir DIR]"""
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

V, BATCH_ROWS = 34, 16 * 334


def time_op(eng, lp, w, pieces, repeat):
    """{piece: ((median, min) ms of the whole stream, (median, min) ms of its END call, tokens)} of one stream over ``lp`` in calls of
    ``piece`` rows, BEGIN .. END, for each piece size of ``pieces``: device events around the launches, the variants INTERLEAVED
    (every round runs each once, in turn).  The stream object (its state with the node pool and the result: two allocations and two
    fills) is made outside the events."""
    def run(piece, timed):
        s = eng.beam_stream(w, lp.shape[0])
        torch.cuda.synchronize()
        a, b, c = (torch.cuda.Event(enable_timing=True) for _ in range(3))
        a.record()
        for r in range(0, lp.shape[0], piece):
            s.push(lp[r:r + piece])
        b.record()
        out = s.finish()
        c.record()
        c.synchronize()
        if timed:
            ms[piece].append(a.elapsed_time(c))
            end[piece].append(b.elapsed_time(c))
        return out
    ms, end, count = {piece: [] for piece in pieces}, {piece: [] for piece in pieces}, {}
    for r in range(repeat + 1):                               # (round 0 warms up and is dropped)
        for piece in pieces:
            count[piece] = run(piece, r > 0).host()["count"]
    return {piece: ((statistics.median(ms[piece]), min(ms[piece])), (statistics.median(end[piece]), min(end[piece])), count[piece])
            for piece in pieces}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=int, default=3600)
    ap.add_argument("--repeat", type=int, default=9)
    ap.add_argument("--layers", type=int, default=16)
    ap.add_argument("--beam", type=int, default=8, help="the model call's beam width")
    ap.add_argument("--dir", default=None, help="where the generated file goes (default: the system's temporary directory)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise _lib.GigaAMHipError("beam_stream_bench needs the GPU: a CPU run measures nothing")
    rng = np.random.default_rng(0)
    model = gigaam_amd.model_from_checkpoint(synth.make_checkpoint("v2_ctc", seed=1, n_layers=args.layers), "cuda:0")
    eng = model.head.engine
    frames = args.seconds * 25

    # (a) the search alone
    x = rng.standard_normal((frames, V)).astype(np.float32)
    np.put_along_axis(x, np.where(rng.random(frames) < 0.6, V - 1, rng.integers(0, V, frames))[:, None], 9.0, axis=1)
    lp = torch.log_softmax(torch.from_numpy(x), dim=-1).to("cuda:0")
    eng.set_hotwords([])
    eng.set_lm(None)
    for w in (4, 8, 32):
        variants = {frames: "one call", BATCH_ROWS: f"calls of {BATCH_ROWS} rows"}
        for piece, ((med, lo), (emed, elo), count) in time_op(eng, lp, w, list(variants), args.repeat).items():
            print(json.dumps({"what": "op_ctc_beam_stream alone, " + variants[piece], "frames": frames, "V": V, "W": w, "tokens": count,
                              "ms_median": round(med, 3), "ms_min": round(lo, 3), "us_per_frame": round(med * 1e3 / frames, 4),
                              "end_call_ms_median": round(emed, 3), "end_call_ms_min": round(elo, 3)}), flush=True)
    del lp

    # (b) the model call against the greedy call it shares the encode + stitch with
    audio = workloads.config5_audio(args.seconds)
    search = dict(vad="windows", stream_search=True, beam_size=args.beam)
    calls = {
        "transcribe_longform(vad='windows') [greedy: shared encode + stitch]": (None, lambda p: model.transcribe_longform(p, vad="windows")),
        "transcribe_longform(vad='windows', stream_search=True), overlap on": ("1", lambda p: model.transcribe_longform(p, **search)),
        "transcribe_longform(vad='windows', stream_search=True), overlap off": ("0", lambda p: model.transcribe_longform(p, **search)),
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
                    os.environ["GAM_BEAM_STREAM_OVERLAP"] = env
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                out = fn(path)
                torch.cuda.synchronize()
                if r:
                    times[name].append(time.perf_counter() - t0)
                os.environ.pop("GAM_BEAM_STREAM_OVERLAP", None)
        base = None
        for name, ts in times.items():
            med = statistics.median(ts)
            base = med if base is None else base
            print(json.dumps({"what": name, "audio_s": args.seconds, "layers": args.layers, "W": args.beam, "s_median": round(med, 4),
                              "s_min": round(min(ts), 4), "s_max": round(max(ts), 4), "added_ms_over_greedy": round((med - base) * 1e3, 2)}),
                  flush=True)
        del out


if __name__ == "__main__":
    main()
