"""Token confidence over a whole recording (gam_op_ctc_confidence_long): what the long pass costs at one hour.
(a) ``op_ctc_confidence_long`` alone on synthetic log-probs [90 000, V] for V = 34 and V = 1025 with the stream's greedy token list
(``op_ctc_greedy_long``'s device result), and the worst case -- ONE token whose run is all 90 000 frames, the serial span walk -- by
device events around the launches, the variants interleaved; (b) the batch pass ``op_ctc_confidence`` on the 32 x 501 x 34 batch with
its greedy lists, the same way (the figures DESIGN.md 4.15 left open); (c) on ``workloads.config5_audio``,
``confidence_longform(vad="windows")`` against ``transcribe_longform(vad="windows", word_timestamps=True)`` of the same file in the
same session -- the encode, stitch and decode the two share --, a host clock around calls that end in a device-to-host copy, the two
interleaved.  What counts there is the ADDED wall time.  A tool, not a test: no threshold; one JSON line per measurement.

    timeout -k 10 900 python tools/confidence_long_bench.py [--seconds 3600] [--repeat 5] [--layers 16] [--dir DIR]"""
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

T_HOUR = 90000


def peaked(rng, shape, v, blank_share=0.6):
    """Log-probs f32 of ``shape`` + [v] whose peak is the blank in ``blank_share`` of the frames, any class elsewhere."""
    x = rng.standard_normal((*shape, v)).astype(np.float32)
    np.put_along_axis(x, np.where(rng.random(shape) < blank_share, v - 1, rng.integers(0, v, shape))[..., None], 9.0, axis=-1)
    return torch.log_softmax(torch.from_numpy(x), dim=-1).to("cuda:0")


def time_events(variants, repeat):
    """{name: (median, min, max) ms} of ``variants`` {name: fn}: device events around each fn's launches, the variants INTERLEAVED
    (every round runs each once, in turn); round 0 warms up and is dropped."""
    ms = {name: [] for name in variants}
    for r in range(repeat + 1):
        for name, fn in variants.items():
            torch.cuda.synchronize()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            if r:
                ms[name].append(a.elapsed_time(b))
    return {name: (statistics.median(v), min(v), max(v)) for name, v in ms.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=int, default=3600)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--layers", type=int, default=16)
    ap.add_argument("--dir", default=None, help="where the generated file goes (default: the system's temporary directory)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise _lib.GigaAMHipError("confidence_long_bench needs the GPU: a CPU run measures nothing")
    rng = np.random.default_rng(0)
    model = gigaam_amd.model_from_checkpoint(synth.make_checkpoint("v2_ctc", seed=1, n_layers=args.layers), "cuda:0")
    eng = model.head.engine

    # (a) the long op alone: a greedy list, and one token that owns every frame
    for v in (34, 1025):
        lp = peaked(rng, (T_HOUR,), v)
        dec = eng.op_ctc_greedy_long(lp)
        tokens = int(dec.counts.cpu()[0])
        one = torch.full((T_HOUR, v), -12.0, device="cuda:0")
        one[:, 3] = -1e-3                                        # the argmax of every frame is class 3
        variants = {}
        for measure in ("prob", "entropy"):
            variants[f"greedy list, {measure}/mean"] = lambda m=measure: eng.op_ctc_confidence_long(lp, dec, measure=m)
        tid, tfr, tcnt = (torch.tensor([x], dtype=torch.int32, device="cuda:0") for x in (3, 0, 1))      # (uploaded outside the events)
        variants["ONE token of 90 000 frames (the serial walk), prob/mean"] = lambda: eng.op_ctc_confidence_long(one, tid, tfr, tcnt)
        for name, (med, lo, hi) in time_events(variants, args.repeat).items():
            print(json.dumps({"what": "op_ctc_confidence_long alone, " + name, "frames": T_HOUR, "V": v,
                              "tokens": 1 if name.startswith("ONE") else tokens, "ms_median": round(med, 4), "ms_min": round(lo, 4),
                              "ms_max": round(hi, 4), "log_probs_MB": round(T_HOUR * v * 4 / 1e6, 1)}), flush=True)
        h = eng.op_ctc_confidence_long(one, [3], [0]).host()
        assert h["status"].tolist() == [1] and h["span"].tolist() == [[T_HOUR]]
        del lp, one, dec

    # (b) the batch pass on the flagship batch's shape
    b, tp, v = 32, 501, 34
    lp = peaked(rng, (b, tp), v)
    enc_len = torch.full((b,), tp, dtype=torch.int32, device="cuda:0")
    dec = eng.op_ctc_beam(lp, enc_len, 1)                        # (a device token list per utterance: width 1)
    variants = {f"{m}/mean": (lambda m=m: eng.op_ctc_confidence(lp, enc_len, dec, measure=m)) for m in ("prob", "entropy")}
    for name, (med, lo, hi) in time_events(variants, max(args.repeat, 20)).items():
        print(json.dumps({"what": "op_ctc_confidence (batch), " + name, "B": b, "T": tp, "V": v, "ms_median": round(med, 4),
                          "ms_min": round(lo, 4), "ms_max": round(hi, 4)}), flush=True)
    del lp, dec

    # (c) the whole call against the call it is pinned to
    audio = workloads.config5_audio(args.seconds)
    calls = {
        "transcribe_longform(vad='windows', word_timestamps=True) [shared]": lambda p: model.transcribe_longform(p, word_timestamps=True, vad="windows"),
        "confidence_longform(vad='windows')": lambda p: model.confidence_longform(p, vad="windows"),
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
            for name, fn in calls.items():                    # interleaved: each round runs the two once
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                out = fn(path)
                torch.cuda.synchronize()
                if r:
                    times[name].append(time.perf_counter() - t0)
        base = None
        for name, ts in times.items():
            med = statistics.median(ts)
            base = med if base is None else base
            print(json.dumps({"what": name, "audio_s": args.seconds, "layers": args.layers, "s_median": round(med, 4),
                              "s_min": round(min(ts), 4), "s_max": round(max(ts), 4), "added_ms_over_shared": round((med - base) * 1e3, 2)}),
                  flush=True)
        del out


if __name__ == "__main__":
    main()
