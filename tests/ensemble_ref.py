"""Host reference of ``ryd_ensemble_diag`` (tests/test_gpu_mc_ensemble.py), in ``np.longdouble``.

Plain NumPy in the style of tests/observe_ref.py, whose ``ket_probabilities``, ``LD`` and ``U53`` it uses; nothing
here calls into ``pulser_amd.engine``.
"""
from __future__ import annotations

import numpy as np

from observe_ref import LD, U53, ket_probabilities


def ref_diag(states, start):
    """(diag, S_abs): ``diag[i, x] = start[i, x] + sum_b |states[i, b, x]|^2`` for ``states`` [T, B, D] and ``start``
    [T, D], every square and sum in longdouble; ``S_abs`` [T, D] is the sum of the absolute values of the summands
    (|start| and the squares), the scale of the rounding bound."""
    states = np.asarray(states)
    start = np.asarray(start).astype(LD)
    assert states.ndim == 3 and start.shape == (states.shape[0], states.shape[2])
    p = ket_probabilities(states).sum(axis=1, dtype=LD)
    return start + p, np.abs(start) + p


# ---------------------------------------------------------------------------------------------------------------------
# The project's tol_sum rule (tests/observe_ref.py): an entry is a sum of n_batch + 1 float64 summands (the value found
# and one square per trajectory) in some order: at most n_batch u S_abs, u = 2^-53; forming x^2 + y^2 costs a few u more
# per term: (n_batch + 8) u S_abs.  (Gradual underflow is not covered by a relative bound: inputs whose squares fall
# below 2^-1022 are chosen so that those squares are exact.)
# ---------------------------------------------------------------------------------------------------------------------
def tol_diag(n_batch, s_abs):
    return (n_batch + 8) * U53 * np.asarray(s_abs, dtype=np.float64)
