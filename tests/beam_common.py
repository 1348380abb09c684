"""What the beam search tests share (CPU and GPU): the score bar and the comparison against a float64 reference, seeded inputs,
hotword pickers, ARPA text, tokenizers, cached op engines, model builders.  Margins stay with each test module."""
import numpy as np
import torch


def bar(ref):
    return 1e-3 * max(1.0, abs(ref))


def compare(h, b, ref, errs, margin, min_margin):
    """ids / frames exactly and score / logp within the bar if the utterance's margin (``min_margin(ref)``) allows; returns whether
    it qualified."""
    got_ids, got_fr = h["rows"][b]
    if min_margin(ref) <= margin:
        return False
    assert got_ids == ref["ids"], (b, got_ids, ref["ids"])
    assert got_fr == ref["frames"], (b, got_fr, ref["frames"])
    for k in ("score", "logp"):
        e = abs(float(h[k][b]) - ref[k])
        errs[k] = max(errs.get(k, 0.0), e / max(1.0, abs(ref[k])))
        assert e <= bar(ref[k]), (b, k, float(h[k][b]), ref[k])
    return True


def wav_file(tmp_path, seconds, seed):
    import wave
    from gigaam_amd import synth
    wav, _ = synth.synth_audio(1, seconds, seed=seed)
    pcm = (wav[0].numpy() * 32768.0).round().clip(-32768, 32767).astype(np.int16)
    p = str(tmp_path / f"clip{seed}.wav")
    with wave.open(p, "wb") as wf:
        wf.setnchannels(1)
        wf.setsampwidth(2)
        wf.setframerate(16000)
        wf.writeframes(pcm.tobytes())
    return p


def tokenizer(V):
    from gigaam_amd import synth
    from gigaam_amd.decoding import Tokenizer
    return Tokenizer(synth.CHAR_VOCAB if V == 34 else synth._e2e_vocab(V - 1))


def log_probs(rng, B, T, V, kind):
    """Seeded log-probs [B, T, V] (float32, log_softmax units): "peaked" (one dominant class per frame) or "flat" (small logits)."""
    x = rng.standard_normal((B, T, V)).astype(np.float32) * (0.3 if kind == "flat" else 1.0)
    if kind == "peaked":
        top = rng.integers(0, V, (B, T))
        np.put_along_axis(x, top[..., None], 9.0, axis=2)
    return torch.log_softmax(torch.from_numpy(x), dim=-1).numpy()


def encp(rng, B, T, JH, scale=1.0):
    return (rng.standard_normal((B, T, JH)) * scale).astype(np.float32)


def ctc_hotwords(rng, lp, n):
    """n phrases of 2-3 tokens, each token one of the two best non-blank ids of a frame of a run of frames: phrases the beam meets."""
    B, T, _ = lp.shape
    top2 = np.argsort(-lp[:, :, :-1], axis=2, kind="stable")[:, :, :2]
    out = []
    for _ in range(n):
        b, L = int(rng.integers(0, B)), int(rng.integers(2, 4))
        t = int(rng.integers(0, max(T - L, 1)))
        out.append([int(top2[b, min(t + i, T - 1), rng.integers(0, 2)]) for i in range(L)])
    return out


def arpa(rng, words, order, sentences=(), unk=True):
    """ARPA text over ``words`` (strings): every unigram, random bigrams / trigrams plus those of ``sentences``."""
    ng = {1: {w: (-rng.uniform(0.5, 3.0), -rng.uniform(0.0, 1.0)) for w in list(words) + ["<s>", "</s>"] + (["<unk>"] if unk else [])}}
    ng[1]["</s>"] = (ng[1]["</s>"][0], 0.0)
    voc = list(words)
    for n in range(2, order + 1):
        d = {}
        for s in sentences:
            ws = ["<s>"] + list(s) + ["</s>"]
            for i in range(len(ws) - n + 1):
                d[tuple(ws[i:i + n])] = None
        for _ in range(3 * len(voc)):
            d[tuple(["<s>"] * (rng.random() < 0.2) + [voc[rng.integers(0, len(voc))] for _ in range(n)])[:n]] = None
        ng[n] = {k: (-rng.uniform(0.05, 1.5), -rng.uniform(0.0, 0.8) if n < order else 0.0) for k in d}
    lines = ["\\data\\"] + [f"ngram {n}={len(ng[n])}" for n in range(1, order + 1)]
    for n in range(1, order + 1):
        lines += ["", f"\\{n}-grams:"]
        for k, (p, b) in ng[n].items():
            lines.append(f"{p:.4f}\t{' '.join(k if n > 1 else (k,))}" + (f"\t{b:.4f}" if n < order else ""))
    return "\n".join(lines + ["", "\\end\\", ""])


_OP_ENGINES = {}


def ctc_op_engine(owner):
    """An engine without a head for ``op_ctc_beam``, one per test module (``owner``): hotwords and the LM are state on it."""
    if owner not in _OP_ENGINES:
        from gigaam_amd import synth
        from gigaam_amd.engine import HipEngine, build_config
        cfg = synth.model_cfg("v2_ctc")
        eng = HipEngine(build_config(cfg["preprocessor"], cfg["encoder"], None), {}, torch.device("cuda:0"))
        eng.set_gemm_mode("f16x3")
        _OP_ENGINES[owner] = eng
    return _OP_ENGINES[owner]


def run_ctc_op(eng, lp, enc_len, W):
    return eng.op_ctc_beam(torch.from_numpy(np.ascontiguousarray(lp)), torch.tensor(enc_len, dtype=torch.int32), W).host()


def run_rnnt_op(eng, encp, enc_len, W, S):
    return eng.op_rnnt_beam(torch.from_numpy(np.ascontiguousarray(encp)), torch.tensor(enc_len, dtype=torch.int32), W, S).host()


def fullsize_ctc_model():
    import gigaam_amd
    from gigaam_amd import synth
    return gigaam_amd.model_from_checkpoint(synth.make_checkpoint("v2_ctc", seed=0), "cuda:0")


def fullsize_rnnt_model():
    """(model, state dict) of the synthetic full-size v2_rnnt checkpoint."""
    import json
    import os

    import gigaam_amd
    from common import ROOT
    from gigaam_amd import synth
    meta = json.load(open(os.path.join(ROOT, "tests", "golden", "fullsize_meta.json")))["fullsize_v2_rnnt"]
    ck = synth.make_checkpoint("v2_rnnt", seed=0, rnnt_blank_bias=meta.get("blank_bias"))
    return gigaam_amd.model_from_checkpoint(ck, "cuda:0"), ck["state_dict"]


def small_rnnt_model(decoding=None):
    import gigaam_amd
    from gigaam_amd import synth
    ck = synth.make_checkpoint("v2_rnnt", seed=1, n_layers=2, rnnt_blank_bias=12.0)
    if decoding is not None:
        ck["cfg"]["decoding"] = decoding
    return gigaam_amd.model_from_checkpoint(ck, "cuda:0"), ck["state_dict"]


def small_sd(rng, V, H=8, JH=8, D=6, L=1, out_gain=1.0, blank_bias=0.0):
    """A small RNN-T head as a float32 state dict (checkpoint key names)."""
    t = lambda *s, g=1.0: torch.from_numpy((rng.standard_normal(s) * g).astype(np.float32))     # noqa: E731
    sd = {"head.decoder.embed.weight": t(V, H)}
    sd["head.decoder.embed.weight"][V - 1] = 0.0
    for l in range(L):
        for k, s in (("weight_ih", (4 * H, H)), ("weight_hh", (4 * H, H)), ("bias_ih", (4 * H,)), ("bias_hh", (4 * H,))):
            sd[f"head.decoder.lstm.{k}_l{l}"] = t(*s, g=0.5)
    sd["head.joint.enc.weight"], sd["head.joint.enc.bias"] = t(JH, D, g=0.6), t(JH, g=0.2)
    sd["head.joint.pred.weight"], sd["head.joint.pred.bias"] = t(JH, H, g=0.6), t(JH, g=0.2)
    sd["head.joint.joint_net.1.weight"], sd["head.joint.joint_net.1.bias"] = t(V, JH, g=out_gain), t(V, g=0.3)
    sd["head.joint.joint_net.1.bias"][V - 1] += blank_bias
    return sd
