"""CPU: the one-batch software pipeline of the chunked longform routes (gigaam_amd/model.py ``_pipeline``): batch n is launched before
batch n - 1 is brought to the host, and the last one is collected after the loop."""
import pytest

from gigaam_amd.model import _pipeline

ORDER = {
    0: [],
    1: ["launch0", "emit0"],
    3: ["launch0", "launch1", "emit0", "launch2", "emit1", "emit2"],
}


@pytest.mark.parametrize("n", sorted(ORDER))
def test_batch_n_is_launched_before_batch_n_minus_1_is_collected(n):
    calls = []

    def launch(k, batch):
        assert batch == f"batch{k}"
        calls.append(f"launch{k}")
        return k          # (0 is a handle like any other: the helper must not take it for "nothing pending")

    def emit(handle):
        calls.append(f"emit{handle}")

    assert _pipeline((f"batch{k}" for k in range(n)), launch, emit) is None
    assert calls == ORDER[n]
