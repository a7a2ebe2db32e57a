"""Exact rational reference of the exact-sum float mode (float_mode="exact", SCT_FLOAT_EXACT_SUM).

Plain numpy and Python integers; nothing of the engine is imported.  The contract it restates
(sctools_amd/csrc/fixedpt.h, include/sctools_gpu.h):

  a stream sample is x = RN(a / b) as a double, 0 when b == 0 (util.h ratio_rcp); such a record
  still counts in n;
  X = x 2^68 is an integer; an entity keeps S = sum X in 3 lanes and Q = sum X^2 in 5 lanes of
  32-bit limb sums, every lane a plain int64 sum, so lanes of disjoint record sets add;
  mean = RN(S / (n 2^68)), var = RN((n Q - S^2) / (n (n - 1) 2^136)), NaN for n < 2; n <= 0 gives
  mean 0.0 and var NaN.

Streams: 0 = uy_gt30 / uy_len, 1 = gq_gt30 / gq_len, 2 = gq_sum / gq_len, 3 = cy_gt30 / cy_len (the
cell view only: the gene views report CY mean and variance 0.0).
"""
from fractions import Fraction

import numpy as np

SHIFT = 68
M32 = (1 << 32) - 1
N_STREAMS = 4
N_LANES = 8  # 3 of S, 5 of Q
LANE_LIMIT = 1 << 63  # the documented headroom: every lane is a non-negative int64
STREAMS = (("uy_gt30", "uy_len"), ("gq_gt30", "gq_len"), ("gq_sum", "gq_len"), ("cy_gt30", "cy_len"))

# output rows (include/sctools_gpu.h SCT_F_*): the mean and variance column of stream 0..3
MEAN_COL = (0, 2, 4, 10)
VAR_COL = (1, 3, 5, 9)
# partial rows (SCT_P_*): P[0] = n, stream s lanes at 24 + 8 s
P_N = 0
P_FLOAT = 24
NP_ROW = 64


def samples_of(a, b):
    """x = float64(a) / float64(b), the IEEE quotient; 0 where b == 0, for any a"""
    a = np.asarray(a).astype(np.float64)
    b = np.asarray(b).astype(np.float64)
    x = np.zeros(np.broadcast(a, b).shape, np.float64)
    np.divide(a, b, out=x, where=b != 0)
    return x


def fixed(x):
    """X = x 2^68 as a Python int (exact: x is 0 or in [2^-16, 2^16))"""
    f = Fraction(float(x)) * (1 << SHIFT)
    assert f.denominator == 1 and f >= 0, x
    assert f == 0 or (1 << (SHIFT - 16)) <= f < (1 << (SHIFT + 16)), x
    return int(f)


def increments(x):
    """the 8 limb pieces one sample adds (fixedpt.h fx_increments): X in 32, 32 and the rest of its
    bits, X^2 in four 32-bit limbs and the rest (bits >= 128, which fx_increments keeps in 64 bits)"""
    X = fixed(x)
    X2 = X * X
    return [X & M32, (X >> 32) & M32, X >> 64,
            X2 & M32, (X2 >> 32) & M32, (X2 >> 64) & M32, (X2 >> 96) & M32, X2 >> 128]


def lanes_of(samples, counts=None):
    """the canonical 8 lanes of the samples (sample k taken counts[k] times): their increments summed"""
    samples = [float(x) for x in np.asarray(samples, np.float64).ravel()]
    counts = [1] * len(samples) if counts is None else [int(c) for c in counts]
    assert len(counts) == len(samples)
    lanes = [0] * N_LANES
    for x, c in zip(samples, counts):
        for k, v in enumerate(increments(x)):
            lanes[k] += v * c
    return lanes


def S_Q_of(lanes):
    """S = sum lane[k] 2^(32 k), k = 0..2, and Q likewise from lanes 3..7: what the ABI promises to
    be additive, whether or not the lanes carry"""
    lanes = [int(v) for v in lanes]
    assert len(lanes) == N_LANES
    S = sum(lanes[k] << (32 * k) for k in range(3))
    Q = sum(lanes[3 + k] << (32 * k) for k in range(5))
    return S, Q


def normalised(lanes):
    """the same S and Q with carries propagated: every lane but the top one of S and of Q below 2^32"""
    S, Q = S_Q_of(lanes)
    return [S & M32, (S >> 32) & M32, S >> 64,
            Q & M32, (Q >> 32) & M32, (Q >> 64) & M32, (Q >> 96) & M32, Q >> 128]


def in_headroom(lanes):
    return all(0 <= int(v) < LANE_LIMIT for v in lanes)


def expected(n, S, Q):
    """(mean, var) correctly rounded from the exact rationals (Fraction.__float__ rounds correctly)"""
    nan = float("nan")
    if n <= 0:
        return 0.0, nan
    mean = float(Fraction(S, n << SHIFT))
    if n < 2:
        return mean, nan
    return mean, float(Fraction(n * Q - S * S, (n * (n - 1)) << (2 * SHIFT)))


def runs_of(col):
    """(run index of every record, number of runs) of an entity column in file order"""
    col = np.asarray(col)
    start = np.ones(col.shape[0], bool)
    start[1:] = col[1:] != col[:-1]
    ent = np.cumsum(start) - 1
    return ent.astype(np.int64), (int(ent[-1]) + 1 if col.shape[0] else 0)


class Sums:
    """n, S and Q of every entity and stream, as Python ints: n[e], S[e][st], Q[e][st]"""

    def __init__(self, n_ent):
        self.n_ent = n_ent
        self.n = [0] * n_ent
        self.S = [[0] * N_STREAMS for _ in range(n_ent)]
        self.Q = [[0] * N_STREAMS for _ in range(n_ent)]

    def floats(self, cell):
        """(mean, var) float64 [n_ent, 4]; the gene views (cell False) report CY as 0.0, 0.0"""
        mean = np.zeros((self.n_ent, N_STREAMS))
        var = np.zeros((self.n_ent, N_STREAMS))
        for e in range(self.n_ent):
            for st in range(N_STREAMS if cell else 3):
                mean[e, st], var[e, st] = expected(self.n[e], self.S[e][st], self.Q[e][st])
        return mean, var


def sums_of(arrays, ent, n_ent, streams=N_STREAMS):
    """Sums of the records' streams grouped by `ent` (an entity index < n_ent per record).  Records
    are grouped by (entity, a, b) first, so a shard costs one big-integer step per distinct triple."""
    ent = np.asarray(ent).astype(np.int64)
    out = Sums(n_ent)
    if ent.shape[0] == 0:
        return out
    assert ent.min() >= 0 and ent.max() < n_ent and n_ent < (1 << 31)
    for e, c in zip(*np.unique(ent, return_counts=True)):
        out.n[int(e)] = int(c)
    cache = {}
    for st in range(streams):
        a = np.asarray(arrays[STREAMS[st][0]]).astype(np.int64)
        b = np.asarray(arrays[STREAMS[st][1]]).astype(np.int64)
        assert a.min() >= 0 and a.max() < (1 << 16) and b.min() >= 0 and b.max() < (1 << 16)
        keys, counts = np.unique((ent << 32) | (a << 16) | b, return_counts=True)
        ka, kb = (keys >> 16) & 0xFFFF, keys & 0xFFFF
        xs = samples_of(ka, kb)
        for e, x, c in zip((keys >> 32).tolist(), xs.tolist(), counts.tolist()):
            v = cache.get(x)
            if v is None:
                X = fixed(x)
                v = cache[x] = (X, X * X)
            out.S[e][st] += v[0] * c
            out.Q[e][st] += v[1] * c
    return out


def naive_sums_of(arrays, ent, n_ent, streams=N_STREAMS):
    """the same sums one record at a time with Fractions: the check of sums_of's grouping"""
    out = Sums(n_ent)
    for i, e in enumerate(np.asarray(ent).tolist()):
        out.n[e] += 1
        for st in range(streams):
            a, b = int(arrays[STREAMS[st][0]][i]), int(arrays[STREAMS[st][1]][i])
            x = Fraction(float(np.float64(a) / np.float64(b))) if b else Fraction(0)
            X = x * (1 << SHIFT)
            assert X.denominator == 1
            out.S[e][st] += int(X)
            out.Q[e][st] += int(X) ** 2
    return out


def top_bit(d):
    """position of the highest set bit of |d| (-1 for 0)"""
    return abs(int(d)).bit_length() - 1
