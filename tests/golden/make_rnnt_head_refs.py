"""Writes tests/golden/rnnt_head_refs.npz: the float64 references of the sets of tests/rnnt_head_cases.py (minutes of CPU; a process
per set).  Run from the repository root: python tests/golden/make_rnnt_head_refs.py.  tests/test_rnnt_head_cases_host.py computes
every set again and compares."""
import os
import sys
from multiprocessing import Pool

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import rnnt_head_cases as H      # noqa: E402


def _job(key):
    return H.set_key(*key), H.compute_set(*key)


if __name__ == "__main__":
    with Pool(min(16, os.cpu_count() or 1)) as pool:
        data = dict(pool.map(_job, H.all_sets(), chunksize=1))
    data["edge"] = H.compute_edge(data[H.set_key("beam", "A", 2, H.EDGE_KIND)][-1]["refs"])
    H.write_refs(data)
    print("wrote", H.REFS_PATH, os.path.getsize(H.REFS_PATH), "bytes")
