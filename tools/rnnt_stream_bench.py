"""RNN-T greedy decode over a whole recording (gam_op_rnnt_greedy_stream): what the resumable one-workgroup decode costs
at one hour.  (a) ``op_rnnt_greedy_stream`` alone on synthetic encp [90 000, joint_hidden] for a V = 34 head (v2_rnnt's) and a
V = 1025 head (v3_e2e_rnnt's) on encp = 3 x standard normal, the head's blank bias picked among 12 .. 30 on the first 3000 frames so
that the token rate is nearest to speech's (about 35 000 tokens an hour, 0.39 a frame), as ONE
call and as calls of one window batch's rows (16 windows x 334 kept frames: 17 calls), by device events around the launches, the two
variants interleaved; (b) on ``workloads.config5_audio`` with the full-size ``v2_rnnt``: ``transcribe_longform(vad="windows",
stream_decode=True)`` with the decode on the decode side stream (the default) and on the launch stream (GAM_RNNT_STREAM_OVERLAP=0),
the same model over ``speech_regions=`` that tile the file in 20 s chunks (the route RNN-T heads had before), and ``v2_ctc`` with
``vad="windows"`` (the encode + stitch of the same windows, a decode that costs next to nothing) -- a host clock around calls that end
in a device-to-host copy, the four interleaved.  A tool, not a test: no threshold; one JSON line per measurement.

    python tools/rnnt_stream_bench.py [--seconds 3600] [--repeat 9] [--layers 16] [--dir DIR] [--skip-model]"""
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
from gigaam_amd.engine import HipEngine, build_config  # noqa: E402

BATCH_ROWS = 16 * 334
ENCP_SCALE, TOKENS_PER_FRAME = 3.0, 35000 / 90000
BIASES = (12.0, 14.0, 16.0, 18.0, 20.0, 22.0, 24.0, 27.0, 30.0)


def head_engine(name, bias, dev):
    cfg = synth.model_cfg(name, n_layers=1)
    return HipEngine(build_config(cfg["preprocessor"], cfg["encoder"], cfg["head"]), synth.make_state_dict(cfg, seed=0, rnnt_blank_bias=bias), dev)


def pick_bias(name, encp, max_symbols, dev):
    """(the blank bias of ``BIASES`` whose token rate on the first rows of ``encp`` is nearest to speech's, that rate)"""
    best = None
    for bias in BIASES:
        eng = head_engine(name, bias, dev)
        s = eng.rnnt_greedy_stream(encp.shape[0], max_symbols)
        s.push(encp)
        rate = len(HipEngine.collect(s.finish())[0][0][0]) / encp.shape[0]
        eng.close()
        if best is None or abs(rate - TOKENS_PER_FRAME) < abs(best[1] - TOKENS_PER_FRAME):
            best = (bias, rate)
    return best


def time_op(eng, encp, max_symbols, pieces, repeat):
    """{piece: ((median, min) ms of the whole stream, tokens)} of one stream over ``encp`` in calls of ``piece`` rows, BEGIN .. END, for
    each piece size of ``pieces``: device events around the launches, the variants INTERLEAVED (every round runs each once, in turn).
    The stream object (its state and its result) is made outside the events."""
    def run(piece, timed):
        s = eng.rnnt_greedy_stream(encp.shape[0], max_symbols)
        torch.cuda.synchronize()
        a, b = (torch.cuda.Event(enable_timing=True) for _ in range(2))
        a.record()
        for r in range(0, encp.shape[0], piece):
            s.push(encp[r:r + piece])
        out = s.finish()
        b.record()
        b.synchronize()
        if timed:
            ms[piece].append(a.elapsed_time(b))
        rows, _ = HipEngine.collect(out)
        s.check()
        return len(rows[0][0])
    ms, count = {piece: [] for piece in pieces}, {}
    for r in range(repeat + 1):                               # (round 0 warms up and is dropped)
        for piece in pieces:
            count[piece] = run(piece, r > 0)
        print(f"round {r}: {count}", file=sys.stderr, flush=True)
    return {piece: ((statistics.median(ms[piece]), min(ms[piece])), count[piece]) for piece in pieces}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=int, default=3600)
    ap.add_argument("--repeat", type=int, default=9)
    ap.add_argument("--layers", type=int, default=16)
    ap.add_argument("--max-symbols", type=int, default=10)
    ap.add_argument("--dir", default=None, help="where the generated file goes (default: the system's temporary directory)")
    ap.add_argument("--skip-model", action="store_true", help="part (a) only")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise _lib.GigaAMHipError("rnnt_stream_bench needs the GPU: a CPU run measures nothing")
    dev = torch.device("cuda:0")
    frames = args.seconds * 25

    # (a) the kernel alone
    for name in ("v2_rnnt", "v3_e2e_rnnt"):
        jh = int(synth.model_cfg(name, n_layers=1)["head"]["joint"]["joint_hidden"])
        encp = torch.from_numpy((np.random.default_rng(0).standard_normal((frames, jh)) * ENCP_SCALE).astype(np.float32)).to(dev)
        bias, rate = pick_bias(name, encp[:3000], args.max_symbols, dev)
        print(f"{name}: blank bias {bias}, {rate:.3f} tokens a frame on 3000 frames", file=sys.stderr, flush=True)
        eng = head_engine(name, bias, dev)
        v = int(eng.cfg.num_classes)
        variants = {frames: "one call", BATCH_ROWS: f"calls of {BATCH_ROWS} rows"}
        for piece, ((med, lo), count) in time_op(eng, encp, args.max_symbols, list(variants), args.repeat).items():
            print(json.dumps({"what": "op_rnnt_greedy_stream alone, " + variants[piece], "head": name, "frames": frames, "V": v, "H": int(eng.cfg.pred_hidden),
                              "JH": jh, "blank_bias": bias, "max_symbols": args.max_symbols, "tokens": count, "ms_median": round(med, 3), "ms_min": round(lo, 3),
                              "us_per_frame": round(med * 1e3 / frames, 4), "us_per_token": round(med * 1e3 / max(count, 1), 4)}), flush=True)
        del encp
        eng.close()
    if args.skip_model:
        return

    # (b) the model call: the new route, the route RNN-T heads had, and the CTC head over the same windows
    rnnt = gigaam_amd.model_from_checkpoint(synth.make_checkpoint("v2_rnnt", seed=1, n_layers=args.layers, rnnt_blank_bias=12.0), "cuda:0")
    ctc = gigaam_amd.model_from_checkpoint(synth.make_checkpoint("v2_ctc", seed=1, n_layers=args.layers), "cuda:0")
    audio = workloads.config5_audio(args.seconds)
    tiles = [(float(a), float(min(a + 20, args.seconds))) for a in range(0, args.seconds, 20)]
    stream = dict(vad="windows", stream_decode=True)
    calls = {
        "v2_ctc transcribe_longform(vad='windows') [greedy CTC over the same windows]": (None, lambda p: ctc.transcribe_longform(p, vad="windows")),
        "v2_rnnt transcribe_longform(vad='windows', stream_decode=True), overlap on": ("1", lambda p: rnnt.transcribe_longform(p, **stream)),
        "v2_rnnt transcribe_longform(vad='windows', stream_decode=True), overlap off": ("0", lambda p: rnnt.transcribe_longform(p, **stream)),
        "v2_rnnt transcribe_longform(speech_regions=20 s tiles) [the route before]": (None, lambda p: rnnt.transcribe_longform(p, speech_regions=tiles)),
    }
    with tempfile.TemporaryDirectory(dir=args.dir) as d:
        path = os.path.join(d, "hour.wav")
        with wave.open(path, "wb") as wf:
            wf.setnchannels(1)
            wf.setsampwidth(2)
            wf.setframerate(16000)
            wf.writeframes((audio.numpy() * 32768.0).round().clip(-32768, 32767).astype(np.int16).tobytes())
        del audio
        times, chars = {name: [] for name in calls}, {}
        for r in range(args.repeat + 1):                      # (round 0 warms every shape up and is dropped)
            for name, (env, fn) in calls.items():             # interleaved: each round runs the four once
                if env is not None:
                    os.environ["GAM_RNNT_STREAM_OVERLAP"] = env
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                out = fn(path)
                torch.cuda.synchronize()
                if r:
                    times[name].append(time.perf_counter() - t0)
                chars[name] = sum(len(s.text) for s in out.segments)
                os.environ.pop("GAM_RNNT_STREAM_OVERLAP", None)
                print(f"round {r}: {name}: {time.perf_counter() - t0:.3f} s", file=sys.stderr, flush=True)
        base = None
        for name, ts in times.items():
            med = statistics.median(ts)
            base = med if base is None else base
            print(json.dumps({"what": name, "audio_s": args.seconds, "layers": args.layers, "chars": chars[name], "s_median": round(med, 4),
                              "s_min": round(min(ts), 4), "s_max": round(max(ts), 4), "added_ms_over_ctc_windows": round((med - base) * 1e3, 2)}),
                  flush=True)


if __name__ == "__main__":
    main()
