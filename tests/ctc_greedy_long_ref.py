"""numpy reference of the CTC greedy decode of one utterance (reference gigaam/decoding.py:56-96): per-frame argmax that takes the FIRST
maximum (torch's tie rule; numpy's argmax has the same), blank = V - 1, keep frame t iff its label is no blank and differs from the
label of frame t - 1.  Helper of tests/test_hip_ctc_greedy_long.py and tests/test_hip_longform_windows.py."""
import numpy as np


def labels_ref(lp):
    lp = np.asarray(lp)
    return lp.argmax(axis=1).astype(np.int64) if lp.shape[0] else np.zeros((0,), np.int64)


def collapse_ref(lab, blank):
    """labels [T] -> (ids, frames) as int lists."""
    lab = np.asarray(lab, dtype=np.int64)
    if lab.shape[0] == 0:
        return [], []
    prev = np.concatenate([[-1], lab[:-1]])
    keep = (lab != blank) & (lab != prev)
    frames = np.nonzero(keep)[0]
    return lab[frames].tolist(), frames.tolist()


def greedy_ref(lp):
    """log-probs [T, V] -> (ids, frames)."""
    lp = np.asarray(lp)
    return collapse_ref(labels_ref(lp), lp.shape[1] - 1)
