"""RNN-T beam search over a whole recording (gam_op_rnnt_beam_stream): what the resumable one-workgroup search costs.
(a) ``op_rnnt_beam_stream`` alone on synthetic encp [frames, joint_hidden] = 3 x standard normal for a V = 34 head (v2_rnnt's) and a
V = 1025 head (v3_e2e_rnnt's), the blank bias picked as tools/rnnt_stream_bench.py picks it (a token rate near speech's), at
W = 4 and 8, without hotwords, with 100 hotwords and with an n-gram LM, as ONE call and as calls of one window batch's rows, by device
events around the launches, the variants interleaved; the END call (final pick and backtrack) alone by events around ``finish``.
(b) on ``workloads.config5_audio`` with the full-size ``v2_rnnt``: ``transcribe_longform(vad="windows", stream_decode="beam")`` after
``set_decoding(beam_size=4)`` with the pushes on the decode side stream (the default) and on the launch stream
(GAM_RNNT_STREAM_OVERLAP=0), beside ``stream_decode=True`` (greedy) on the same file -- a host clock around calls that end in a
device-to-host copy, the three interleaved.  A tool, not a test: no threshold; one JSON line per measurement.

    python tools/rnnt_beam_stream_bench.py [--op-seconds 600] [--seconds 3600] [--repeat 5] [--layers 16] [--dir DIR] [--skip-model] [--skip-op]"""
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
sys.path.insert(0, os.path.join(ROOT, "tools"))

import gigaam_amd  # noqa: E402
from gigaam_amd import _lib, synth, workloads  # noqa: E402
from gigaam_amd import lm as LM  # noqa: E402
from gigaam_amd.decoding import Tokenizer  # noqa: E402
from rnnt_stream_bench import BATCH_ROWS, ENCP_SCALE, head_engine, pick_bias  # noqa: E402


def tokenizer(name, v):
    return Tokenizer(synth.CHAR_VOCAB if name == "v2_rnnt" else synth._e2e_vocab(v - 1))


def small_lm(tok, v, d):
    """An order-3 LM over 200 random words the tokenizer spells back (uniform-ish random probabilities): the search then makes the
    queries of a real one -- one per new hypothesis with a non-empty partial word."""
    rng = np.random.default_rng(5)
    words = set()
    while len(words) < 200:
        w = tok.decode([int(c) for c in rng.integers(0, v - 1, int(rng.integers(2, 6)))]).replace("▁", " ").strip()
        if w and " " not in w:
            words.add(w)
    words = sorted(words)
    lines, grams = ["\\data\\"], {1: [(w,) for w in words + ["<s>", "</s>", "<unk>"]]}
    for n in (2, 3):
        grams[n] = sorted({tuple(words[int(i)] for i in rng.integers(0, len(words), n)) for _ in range(600)})
    lines += [f"ngram {n}={len(grams[n])}" for n in (1, 2, 3)]
    for n in (1, 2, 3):
        lines += ["", f"\\{n}-grams:"]
        for g in grams[n]:
            lines.append(f"{-rng.uniform(0.3, 3.0):.4f}\t{' '.join(g)}" + (f"\t{-rng.uniform(0.0, 0.8):.4f}" if n < 3 else ""))
    path = os.path.join(d, "bench.arpa")
    with open(path, "w", encoding="utf-8") as f:
        f.write("\n".join(lines + ["", "\\end\\", ""]))
    return LM.NgramLM.from_arpa(path)


def time_op(eng, encp, w, max_symbols, pieces, repeat):
    """{piece: ((median, min) ms of the pushes, (median, min) ms of the END call, tokens)} of one stream over ``encp`` in calls of
    ``piece`` rows: device events around the launches, the variants INTERLEAVED.  The stream object is made outside the events."""
    def run(piece, timed):
        s = eng.rnnt_beam_stream(w, encp.shape[0], max_symbols)
        torch.cuda.synchronize()
        a, b, c = (torch.cuda.Event(enable_timing=True) for _ in range(3))
        a.record()
        for r in range(0, encp.shape[0], piece):
            s.push(encp[r:r + piece])
        b.record()
        out = s.finish()
        c.record()
        c.synchronize()
        if timed:
            ms[piece].append(a.elapsed_time(b))
            end[piece].append(b.elapsed_time(c))
        return out.host()["count"]
    ms, end, count = {p: [] for p in pieces}, {p: [] for p in pieces}, {}
    for r in range(repeat + 1):                               # (round 0 warms up and is dropped)
        for piece in pieces:
            count[piece] = run(piece, r > 0)
        print(f"round {r}: {count}", file=sys.stderr, flush=True)
    return {p: ((statistics.median(ms[p]), min(ms[p])), (statistics.median(end[p]), min(end[p])), count[p]) for p in pieces}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--op-seconds", type=int, default=600, help="audio seconds of the op-level streams (25 frames a second)")
    ap.add_argument("--seconds", type=int, default=3600)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--layers", type=int, default=16)
    ap.add_argument("--max-symbols", type=int, default=10)
    ap.add_argument("--dir", default=None, help="where the generated files go (default: the system's temporary directory)")
    ap.add_argument("--skip-model", action="store_true", help="part (a) only")
    ap.add_argument("--skip-op", action="store_true", help="part (b) only")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise _lib.GigaAMHipError("rnnt_beam_stream_bench needs the GPU: a CPU run measures nothing")
    dev = torch.device("cuda:0")
    frames = args.op_seconds * 25

    with tempfile.TemporaryDirectory(dir=args.dir) as d:
        # (a) the kernel alone
        for name in () if args.skip_op else ("v2_rnnt", "v3_e2e_rnnt"):
            jh = int(synth.model_cfg(name, n_layers=1)["head"]["joint"]["joint_hidden"])
            encp = torch.from_numpy((np.random.default_rng(0).standard_normal((frames, jh)) * ENCP_SCALE).astype(np.float32)).to(dev)
            bias, rate = pick_bias(name, encp[:3000], args.max_symbols, dev)
            print(f"{name}: blank bias {bias}, {rate:.3f} tokens a frame (greedy) on 3000 frames", file=sys.stderr, flush=True)
            eng = head_engine(name, bias, dev)
            v = int(eng.cfg.num_classes)
            tok = tokenizer(name, v)
            rng = np.random.default_rng(9)
            phrases = [[int(c) for c in rng.integers(0, v - 1, int(rng.integers(2, 5)))] for _ in range(100)]
            lm = small_lm(tok, v, d)
            piece = BATCH_ROWS if frames > BATCH_ROWS else max(frames // 8, 1)      # (a short stream: eight calls)
            variants = {frames: "one call", piece: f"calls of {piece} rows"}
            for w in (4, 8):
                for mode in ("plain", "100 hotwords", "LM"):
                    eng.set_hotwords(phrases if mode == "100 hotwords" else [], 1.5)
                    eng.set_lm(lm if mode == "LM" else None, tok, 0.5, 1.0)
                    for piece, ((med, lo), (emed, elo), count) in time_op(eng, encp, w, args.max_symbols, list(variants), args.repeat).items():
                        print(json.dumps({"what": "op_rnnt_beam_stream alone, " + variants[piece], "head": name, "mode": mode, "W": w, "frames": frames,
                                          "V": v, "H": int(eng.cfg.pred_hidden), "JH": jh, "blank_bias": bias, "max_symbols": args.max_symbols,
                                          "tokens": count, "ms_median": round(med, 3), "ms_min": round(lo, 3),
                                          "us_per_frame": round(med * 1e3 / frames, 3), "end_call_ms_median": round(emed, 3),
                                          "end_call_ms_min": round(elo, 3)}), flush=True)
            del encp
            eng.close()
        if args.skip_model:
            return

        # (b) the model call: the beam route with the side stream on and off, beside the greedy route on the same file
        rnnt = gigaam_amd.model_from_checkpoint(synth.make_checkpoint("v2_rnnt", seed=1, n_layers=args.layers, rnnt_blank_bias=12.0), "cuda:0")
        audio = workloads.config5_audio(args.seconds)

        def beam(p):
            rnnt.set_decoding(beam_size=4)
            try:
                return rnnt.transcribe_longform(p, vad="windows", stream_decode="beam")
            finally:
                rnnt.set_decoding()

        calls = {
            "v2_rnnt transcribe_longform(vad='windows', stream_decode=True) [greedy]": (None, lambda p: rnnt.transcribe_longform(p, vad="windows", stream_decode=True)),
            "v2_rnnt set_decoding(beam_size=4); transcribe_longform(vad='windows', stream_decode='beam'), overlap on": ("1", beam),
            "v2_rnnt set_decoding(beam_size=4); transcribe_longform(vad='windows', stream_decode='beam'), overlap off": ("0", beam),
        }
        path = os.path.join(d, "hour.wav")
        with wave.open(path, "wb") as wf:
            wf.setnchannels(1)
            wf.setsampwidth(2)
            wf.setframerate(16000)
            wf.writeframes((audio.numpy() * 32768.0).round().clip(-32768, 32767).astype(np.int16).tobytes())
        del audio
        times, chars = {name: [] for name in calls}, {}
        for r in range(args.repeat + 1):                      # (round 0 warms every shape up and is dropped)
            for name, (env, fn) in calls.items():             # interleaved: each round runs the three once
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
                              "s_min": round(min(ts), 4), "s_max": round(max(ts), 4), "added_s_over_greedy": round(med - base, 4)}), flush=True)


if __name__ == "__main__":
    main()
