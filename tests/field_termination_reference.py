"""The rank windows of the front-to-back field frame, restated in numpy.  No device.

The rule is the baked frame's (``tests/baked_termination_reference.py``: the rank-k sample contributes iff the fp32 optical
depth accumulated before it satisfies ``cum <= stop_tau``), so the contributing samples of a ray are a prefix of its
samples and ``kept > r`` says that the rule holds for the sample of rank r.  A schedule ``b_1 < ... < b_m`` (``b_0 = 0``)
cuts the ranks into windows ``[b_{j-1}, b_j)``; a ray is EVALUATED in window j iff it has a sample of rank ``b_{j-1}`` and
the rule holds for that sample, and then all of its samples in the window are."""
import numpy as np

from tests.baked_termination_reference import contributing_counts, stop_tau, truncate  # noqa: F401  (one restatement serves both)


def evaluated_counts(counts, kept, windows) -> np.ndarray:
    """Per ray, how many of its samples the field evaluates: ``min(count, b_j)`` for the last window j the ray entered,
    0 for a ray without samples.  ``counts``: samples per ray; ``kept``: ``contributing_counts`` of the same rays;
    ``windows``: the schedule, strictly increasing, first >= 1, last >= every count.  int64 [len(counts)]."""
    counts = np.asarray(counts, dtype=np.int64).reshape(-1)
    kept = np.asarray(kept, dtype=np.int64).reshape(-1)
    windows = [int(b) for b in windows]
    assert counts.shape == kept.shape and (kept <= counts).all() and (kept >= 0).all()
    assert len(windows) >= 1 and windows[0] >= 1 and all(a < b for a, b in zip(windows, windows[1:]))
    assert counts.size == 0 or windows[-1] >= counts.max(), "the last window must reach every sample"
    out = np.zeros(counts.shape, dtype=np.int64)
    start = 0
    for end in windows:
        entered = (counts > start) & (kept > start)          # a sample of rank `start`, and it contributes
        out[entered] = np.minimum(counts[entered], end)
        start = end
    return out
