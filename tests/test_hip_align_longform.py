"""GPU: GigaAMASR.align_longform (forced alignment of a whole transcript against a long recording, gam_op_ctc_align_long) on a
synthetic 2-layer v2_ctc model: the greedy ids of every speech region, concatenated, must come back where the per-region alignment
(align_batch) puts them."""
import numpy as np
import pytest
import torch

from common import report

from test_hip_ctc_align import _bar, _golden_margins, _wav_file

pytestmark = pytest.mark.gpu

REGIONS = [(0.5, 21.5), (24.0, 42.0), (45.0, 68.0)]      # 21 s, 18 s, 23 s: pack_regions keeps them apart; two feeder batches of <= 2
SEED = 31


@pytest.fixture(scope="module")
def longform(tmp_path_factory):
    """The model, the 70 s file, and per region: greedy ids, the per-region alignment, the head's log-probs (computed once)."""
    import gigaam_amd
    from gigaam_amd import synth
    from gigaam_amd.vad_utils import segment_audio_file
    ck = synth.make_checkpoint("v2_ctc", seed=1, n_layers=2)
    model = gigaam_amd.model_from_checkpoint(ck, "cuda:0")
    path = _wav_file(tmp_path_factory.mktemp("longform"), 70.0, SEED)
    segments, bounds = segment_audio_file(path, 16000, speech_regions=REGIONS)
    assert [tuple(b) for b in bounds] == REGIONS
    per = []
    with torch.inference_mode():
        for seg in segments:
            wav, wlen = seg[None, :], torch.tensor([seg.shape[0]])
            enc, elen = model._encode(wav.to("cuda:0"), wlen.to("cuda:0"), wlen)
            ids = model.decoding.decode(model.head, enc, elen)[0][1]
            lp = model.head.engine.ctc_head(enc)[0, : int(elen[0])].double().cpu().numpy()
            al = model.align_batch(wav, wlen, [ids])[0]
            assert al.feasible
            per.append(dict(ids=ids, lp=lp, al=al, frames=int(elen[0])))
    return model, path, per


def test_longform_alignment_of_the_greedy_ids_matches_the_per_region_alignments(longform):
    from gigaam_amd.types import LongformAlignmentResult
    model, path, per = longform
    all_ids = [i for p in per for i in p["ids"]]
    res = model.align_longform(path, all_ids, fr_batch_size=2, speech_regions=REGIONS)
    assert isinstance(res, LongformAlignmentResult) and res.feasible and res.token_ids == all_ids
    assert len(res.segments) == len(REGIONS)
    # a region whose last token equals the next region's first: the per-region paths, concatenated, are no CTC path of the
    # concatenated ids (a blank would have to part the two), so nothing is compared there
    dropped = [k for k in range(len(per) - 1) if per[k]["ids"] and per[k + 1]["ids"] and per[k]["ids"][-1] == per[k + 1]["ids"][0]]
    assert len(dropped) <= 1, dropped
    best = sum(float(p["lp"].max(axis=1).sum()) for p in per)
    parts = sum(p["al"].score for p in per)
    report("align_longform_greedy_ids", score=res.score, sum_of_regions=parts, sum_of_frame_maxima=best, tokens=len(all_ids),
           frames=sum(p["frames"] for p in per), boundaries_dropped=len(dropped))
    print("score", res.score, "regions", parts, "maxima", best, "tokens", len(all_ids), "dropped", dropped)
    assert abs(parts - best) <= _bar(best)
    if not dropped:
        assert abs(res.score - parts) <= _bar(parts)
        assert abs(res.score - best) <= _bar(best)
    assert res.log_likelihood >= res.score - _bar(res.score)
    # every token in its own region, on the per-region frame wherever the frame boundary is not a near-tie
    want_seg = [k for k, p in enumerate(per) for _ in p["ids"]]
    skip = {k for d in dropped for k in (d, d + 1)}
    checked, o = 0, 0
    for k, p in enumerate(per):
        m = _golden_margins(p["lp"])
        for u, f in enumerate(p["al"].token_frames):
            if k not in skip:
                assert res.token_segments[o + u] == k, (k, u)
                if min(m[max(f - 1, 0)], m[f]) > 1e-3:
                    assert res.token_frames[o + u] == f, (k, u)
                    checked += 1
        o += len(p["ids"])
    if not dropped:
        assert res.token_segments == want_seg
    assert checked >= 0.8 * sum(len(p["ids"]) for k, p in enumerate(per) if k not in skip)
    # token times: region start + local frame x that region's frame shift
    for k, f, t in zip(res.token_segments, res.token_frames, res.token_times):
        shift = (REGIONS[k][1] - REGIONS[k][0]) / per[k]["frames"]
        assert t == pytest.approx(REGIONS[k][0] + f * shift, abs=1e-6)
    # words: inside their Segment, monotone.  The greedy ids of two regions are concatenated with no space between them, so the
    # last word of a region runs on into the next one: such a word starts inside its Segment and ends inside the region of its
    # last token (at most one per region boundary)
    from gigaam_amd.timestamps_utils import word_token_groups
    groups = word_token_groups(model.decoding.tokenizer, all_ids)
    assert sum(len(s.words) for s in res.segments) == len(res.words) == len(groups)
    for s, (a, b) in zip(res.segments, REGIONS):
        assert (s.start, s.end) == (a, b)
    straddling = 0
    for w, g in zip(res.words, groups):
        k0, k1 = res.token_segments[g[0]], res.token_segments[g[-1]]
        assert any(w is x for x in res.segments[k0].words)
        if k0 == k1:                        # the rule: a word's times lie inside its Segment
            assert REGIONS[k0][0] - 1e-3 <= w.start < w.end <= REGIONS[k0][1] + 1e-3, (w, k0)
        else:                               # a word that runs on: starts inside its Segment, ends inside its last token's region
            assert REGIONS[k0][0] - 1e-3 <= w.start <= REGIONS[k0][1] + 1e-3, (w, k0)
            assert REGIONS[k1][0] - 1e-3 <= w.end <= REGIONS[k1][1] + 1e-3, (w, k1)
        straddling += k1 != k0
    assert straddling <= len(REGIONS) - 1
    starts = [w.start for w in res.words]
    assert starts == sorted(starts)
    assert all(x.end <= y.start + 1e-3 for x, y in zip(res.words, res.words[1:]))


def test_longform_alignment_of_a_string(longform):
    model, path, _ = longform
    text = "привет мир это проверка выравнивания длинной записи"
    res = model.align_longform(path, text, fr_batch_size=2, speech_regions=REGIONS)
    assert res.feasible and str(res) == text
    assert [w.text for w in res.words] == text.split()
    assert len(res.token_times) == len(res.token_ids) == len(text)
    assert np.isfinite(res.score) and res.log_likelihood >= res.score - 1e-3 * abs(res.score)
    with pytest.raises(ValueError):
        model.align_longform(path, "abc", speech_regions=REGIONS)              # Latin letters: not in the vocabulary
    with pytest.raises(ValueError, match="cannot be aligned"):
        model.align_longform(path, "а" * 2000, speech_regions=REGIONS)         # 3999 frames needed, ~1550 there
    with pytest.raises(ValueError, match="no speech"):
        model.align_longform(path, "а", speech_regions=[])
    eng = model.head.engine
    eng.set_ctc_align_workspace(4096)
    try:
        with pytest.raises(ValueError, match="4096"):
            model.align_longform(path, text, speech_regions=REGIONS)
    finally:
        eng.set_ctc_align_workspace(0)


def test_align_still_refuses_the_long_file(longform):
    model, path, _ = longform
    with pytest.raises(ValueError, match="25 s"):
        model.align(path, "а")


def test_align_longform_needs_a_ctc_head(longform):
    import gigaam_amd
    from gigaam_amd import synth
    _, path, _ = longform
    model = gigaam_amd.model_from_checkpoint(synth.make_checkpoint("v2_rnnt", seed=1, n_layers=1), "cuda:0")
    with pytest.raises(TypeError, match="forced alignment needs a CTC head"):
        model.align_longform(path, "а", speech_regions=REGIONS)
