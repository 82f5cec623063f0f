"""The sampling controls of l2_step_batch_sampling (include/llama2_hip.h: l2_sample_controls) as plain numpy: stage A, the penalties
on tokens already seen (visible: they change the row everything reads), and stage B, top-k and min-p (sampler-only: the row the
sampler draws from).  Every rule is an IEEE operation rounded on its own -- no transcendental but the one log(min_p), which the
library takes from C `log` as math.log does -- so the device is held to these functions bit for bit."""
import math

import numpy as np


def penalise(x, history, repetition=1.0, presence=0.0, frequency=0.0):
    """Stage A.  x' of one fp32 row: for every id j that occurs c_j > 0 times in `history`
        y     = rep == 1 ? x[j] : (x[j] > 0 ? (float)((double)x[j] / rep) : (float)((double)x[j] * rep))
        x'[j] = presence == 0 && frequency == 0 ? y : (float)((double)y - (presence + frequency * (double)c_j))
    and every other entry as it was."""
    out = np.array(x, dtype=np.float32, copy=True)
    rep, pres, freq = float(repetition), float(presence), float(frequency)
    ids, counts = np.unique(np.asarray([] if history is None else history, dtype=np.int64), return_counts=True)
    if rep == 1.0 and pres == 0.0 and freq == 0.0:
        return out
    with np.errstate(all="ignore"):
        for j, c in zip(ids.tolist(), counts.tolist()):
            y = out[j]
            if rep != 1.0:
                y = np.float32(np.float64(y) / np.float64(rep)) if y > 0 else np.float32(np.float64(y) * np.float64(rep))
            if pres != 0.0 or freq != 0.0:
                y = np.float32(np.float64(y) - np.float64(pres + freq * float(c)))
            out[j] = y
    return out


def rank_keys(x):
    """The order of the top lists as one unsigned key per entry (larger ranks first; equal keys by ascending id): the value word of
    the library's argmax key -- -0 counts as +0, a NaN ranks below -inf, except at index 0 where it ranks above +inf."""
    v = np.asarray(x, dtype=np.float32) + np.float32(0.0)
    u = v.view(np.uint32).astype(np.uint64)
    key = np.where(u & 0x80000000, ~u & 0xffffffff, u | 0x80000000)
    nan = np.isnan(v)
    key[nan] = 0
    if v.size and nan[0]:
        key[0] = 0xffffffff
    return key.astype(np.int64)


def top_k_survivors(x, k):
    """Token j survives iff fewer than k tokens rank before it (k <= 0 or k >= V: all survive)."""
    V = np.asarray(x).size
    keep = np.ones(V, dtype=bool)
    if 0 < k < V:
        order = np.lexsort((np.arange(V), -rank_keys(x)))
        keep[:] = False
        keep[order[:k]] = True
    return keep


def min_p_margins(x, temperature, min_p):
    """((double)s_j - (double)s_max) - log(min_p) per entry, s_j = (float)((double)x[j] / T): >= 0 survives (a NaN does not)."""
    with np.errstate(all="ignore"):
        s = (np.asarray(x, dtype=np.float32).astype(np.float64) / np.float64(temperature)).astype(np.float32)
        smax = np.float32(-np.inf) if np.isnan(s).all() else np.fmax.reduce(s)
        return (s.astype(np.float64) - np.float64(smax)) - math.log(min_p)


def truncate(x, temperature, top_k=0, min_p=0.0):
    """Stage B.  x'' of one fp32 row x': a greedy row (temperature 0) and a row with top_k 0 and min_p 0 are copies; otherwise
    x''[j] = x'[j] for a survivor of both tests (each made on x') and -inf for every other entry."""
    out = np.array(x, dtype=np.float32, copy=True)
    if temperature == 0.0 or (top_k <= 0 and min_p <= 0.0):
        return out
    keep = top_k_survivors(out, int(top_k))
    if min_p > 0.0:
        with np.errstate(all="ignore"):
            keep &= min_p_margins(out, temperature, min_p) >= 0.0
    out[~keep] = -np.inf
    return out


def min_p_clearance(x, temperature, min_p):
    """The smallest |(s_j - s_max) - log(min_p)| over the finite margins of a row: a test keeps it above 1e-9, so that a last-place
    difference between two `log` implementations cannot decide a case.  For min_p == 1 the threshold is log(1) = +0 exactly in
    every implementation (C11 F.10.3.7), so the entries that tie the maximum -- margin exactly 0, survivors by an exact comparison
    -- are left out, and every other entry must still clear the margin."""
    m = min_p_margins(x, temperature, min_p)
    m = np.abs(m[np.isfinite(m)])
    if min_p == 1.0:
        m = m[m != 0.0]
    return float(m.min()) if m.size else float("inf")
