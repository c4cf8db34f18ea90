"""Inputs shared by tests/test_seq_k_cpu.py and tests/test_seq_k_gpu.py (per-sequence k_strongest): azimuth rows with a chosen number of
returns at or above z_min, where the zero slots in front of a bearing's K slots and the window [K - k, K) of a k <= K meet."""
import numpy as np

K_MAX = 40
KS = (1, 5, 12)
# returns at or above z_min a handmade row holds: 0, 1, k - 1, k, k + 1 for every k of KS, and K - 1
COUNTS = sorted({0, 1, K_MAX - 1} | {k + d for k in KS for d in (-1, 0, 1)})


def handmade_frames(frames, z_min, seed=5):
    """A copy of frames [T, A, R] (uint8) in which, in every sweep, one azimuth row per entry of COUNTS (another row in every sweep) holds
    exactly that many bytes >= z_min: the rest of the row is pushed below z_min, the returns sit at distinct ranges past the minimum
    distance and take their intensities from three levels only, so that within a row several are equal and the range decides."""
    out = np.array(frames, dtype=np.uint8, copy=True)
    T, A, R = out.shape
    rng = np.random.default_rng(seed)
    levels = np.array([z_min, z_min + 7, 200], dtype=np.uint8)
    for t in range(T):
        rows = rng.choice(A, size=len(COUNTS), replace=False)
        for a, c in zip(rows, COUNTS):
            out[t, a] = np.minimum(out[t, a], z_min - 1)
            at = rng.choice(np.arange(60, R), size=c, replace=False)
            out[t, a, at] = rng.choice(levels, size=c)
            assert int((out[t, a] >= z_min).sum()) == c
    return out

