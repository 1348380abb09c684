"""The six synthetic RNN-T heads of the cluster-decode matrix (tests/test_hip_rnnt_cluster_matrix.py on the GPU,
tests/test_rnnt_cluster_plan_host.py on the CPU): sizes other than pred_hidden = joint_hidden = 320, i.e. the instantiations of
gam_rnnt_cluster_kernel that take the sizes as arguments (gam_api.hip rnnt_cluster_kern[4..8]), and the slicing edges of
gam_decode_cluster.h -- a member with no hidden units and no W_pred rows (D at C = 5, 7), fewer k-quads than k-parts (D), one wave
doing the whole window fetch (D), H != JH (B, C, E, F), LDS next to the 160 KiB limit (F at C = 1).

One seeded state dict and one batch per head.  The batch: encoded [6, d_model, 60], lengths 60, 33, 17, 16, 1, 0 (two windows and
a tail, a window and one frame, exactly one window, one frame, none), max_symbols 3; frames 7..44 of utterance 0 are scaled by
0.02 (the quiet span: the blank bias then wins for more than two 16-frame windows whatever the phase).  The seed and the blank
bias of each head were picked on the CPU with the float64 reference alone (tests/rnnt_beam_ref.py greedy_trace); the host test
asserts what they were picked for."""
import functools

import numpy as np

import rnnt_beam_ref as R

MAX_SYMBOLS = 3
T_MAX = 60
LENGTHS = [60, 33, 17, 16, 1, 0]
QUIET = (7, 45)          # frames [7, 45) of utterance 0
QUIET_SCALE = 0.02

# name -> (V, pred_hidden, joint_hidden, seed, blank bias); beside each: the smallest top-1 / top-2 margin of the six utterances by
# the float64 reference, the longest blank run of utterance 0, frames that emit max_symbols tokens
HEADS = {
    "A": (34, 512, 512, 0, 12.0),     # margin 2.6e-2, blank run 45, 44 capped frames
    "B": (257, 256, 512, 1, 9.0),     # margin 1.2e-2, blank run 38, 80 capped frames
    "C": (34, 48, 64, 2, 9.0),        # margin 5.2e-2, blank run 43, 43 capped frames
    "D": (34, 16, 16, 0, 9.0),        # margin 1.9e-2, blank run 38, 70 capped frames
    "E": (130, 496, 336, 0, 9.0),     # margin 1.5e-2, blank run 38, 76 capped frames
    "F": (1025, 320, 512, 2, 9.0),    # margin 1.8e-2, blank run 38, 88 capped frames
}


def head_cfg(name):
    from gigaam_amd import synth
    V, H, JH = HEADS[name][:3]
    cfg = synth.model_cfg("v2_rnnt", n_layers=1)
    cfg["head"]["decoder"]["num_classes"] = cfg["head"]["joint"]["num_classes"] = V
    cfg["head"]["decoder"]["pred_hidden"] = cfg["head"]["joint"]["pred_hidden"] = H
    cfg["head"]["joint"]["joint_hidden"] = JH
    return cfg


def make_inputs(name, seed, blank_bias):
    """(cfg, state dict, encoded [6, d_model, 60] float32, lengths) of a head at a given seed and blank bias."""
    from gigaam_amd import synth
    cfg = head_cfg(name)
    sd = synth.make_state_dict(cfg, seed=seed, rnnt_blank_bias=blank_bias)
    rng = np.random.default_rng(1000 + seed)
    encoded = rng.standard_normal((len(LENGTHS), cfg["encoder"]["d_model"], T_MAX)).astype(np.float32)
    encoded[0, :, QUIET[0]:QUIET[1]] *= QUIET_SCALE
    return cfg, sd, encoded, list(LENGTHS)


@functools.lru_cache(maxsize=None)
def inputs(name):
    return make_inputs(name, *HEADS[name][3:])


@functools.lru_cache(maxsize=None)
def reference(name):
    """The float64 greedy decode (R.greedy_trace) of the head's six utterances; computed once, shared, not to be changed."""
    _, sd, encoded, lengths = inputs(name)
    head = R.head_from_state_dict(sd, 1)
    return [R.greedy_trace(head, encoded[b], T, MAX_SYMBOLS) for b, T in enumerate(lengths)]


def longest_blank_run(per_frame):
    best = run = 0
    for n in per_frame:
        run = run + 1 if n == 0 else 0
        best = max(best, run)
    return best
