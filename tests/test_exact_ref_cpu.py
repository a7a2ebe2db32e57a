"""tests/exact_ref.py, the exact rational reference of the exact-sum float mode, against the host
build of sctools_amd/csrc/fixedpt.h (tests/native/libfxcheck.so) and against a per-record Fraction loop.

The GPU tests of tests/test_gpu_exact_lanes.py hold the device to exact_ref bit for bit; here the
reference itself is held to the header it restates, at the edges of the documented headroom
(n < 2^31 while x <= 93, x up to 65535 while n <= 2^22), and its record grouping to a naive loop.
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import exact_ref as X

HERE = os.path.dirname(os.path.abspath(__file__))
LIB = os.path.join(HERE, "native", "libfxcheck.so")

N31 = (1 << 31) - 1
N22 = 1 << 22


@pytest.fixture(scope="module")
def fx():
    if not os.path.exists(LIB):
        subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-o", LIB,
                        os.path.join(HERE, "native", "fxcheck.cpp")], check=True)
    lib = ctypes.CDLL(LIB)
    lib.fx_stats.argtypes = [ctypes.c_void_p, ctypes.c_int64, ctypes.POINTER(ctypes.c_double),
                             ctypes.POINTER(ctypes.c_double), ctypes.c_void_p]
    lib.fx_finalize_lanes.argtypes = [ctypes.c_void_p, ctypes.c_int64, ctypes.POINTER(ctypes.c_double),
                                      ctypes.POINTER(ctypes.c_double)]
    return lib


def bits(v):
    return int(np.float64(v).view(np.int64))


def same_float(got, want):
    return (np.isnan(got) and np.isnan(want)) or bits(got) == bits(want)


def host_finalize(fx, lanes, n):
    arr = np.array(lanes, dtype=np.int64)
    m, v = ctypes.c_double(), ctypes.c_double()
    fx.fx_finalize_lanes(arr.ctypes.data, n, ctypes.byref(m), ctypes.byref(v))
    return m.value, v.value


def host_lanes(fx, xs):
    """the header's own lanes of a short sample list (fx_accumulate per sample)"""
    x = np.ascontiguousarray(np.asarray(xs, dtype=np.float64))
    arr = np.zeros(X.N_LANES, dtype=np.int64)
    m, v = ctypes.c_double(), ctypes.c_double()
    fx.fx_stats(x.ctypes.data, x.shape[0], ctypes.byref(m), ctypes.byref(v), arr.ctypes.data)
    return [int(t) for t in arr], m.value, v.value


def q(a, b):
    return float(X.samples_of(a, b))


# (samples, counts) per case
CASES = {
    "n31_of_93": ([93.0], [N31]),
    "93_and_a_third_half_and_half": ([93.0, q(1, 3)], [1 << 30, (1 << 30) - 1]),
    "one_1_65535_among_93s": ([q(1, 65535), 93.0], [1, N31 - 1]),
    "n22_of_65535": ([65535.0], [N22]),
    "n22_of_65535_and_1_65535": ([65535.0, q(1, 65535)], [N22 // 2, N22 // 2]),
    "zero_denominators": ([q(0, 0), q(7, 0), q(65535, 0), q(3, 10)], [5, 3, 1, 2]),
    "only_zero_denominators": ([q(9, 0)], [4]),
    "numerator_above_denominator": ([q(255, 10), q(65535, 2), q(40, 31), q(512, 511)], [3, 1, 9, 2]),
    "one_sample": ([q(2, 7)], [1]),
    "two_samples": ([q(2, 7), q(5, 9)], [1, 1]),
    "constant": ([q(9, 10)], [1000]),
}


def random_case(seed):
    rng = np.random.default_rng(1000 + seed)
    k = int(rng.integers(1, 40))
    b = rng.integers(0 if seed % 5 == 0 else 1, 1 << 16, k)
    a = rng.integers(0, 1 << 16, k)
    if seed % 3 == 0:  # quality fractions: a <= b
        a = rng.integers(0, b + 1)
    counts = rng.integers(1, 1 << (1 + seed % 10), k)
    return X.samples_of(a, b).tolist(), counts.tolist()


def check_case(fx, samples, counts):
    n = int(sum(counts))
    lanes = X.lanes_of(samples, counts)
    assert X.in_headroom(lanes)
    S, Q = X.S_Q_of(lanes)
    assert S == sum(X.fixed(x) * c for x, c in zip(samples, counts))
    assert Q == sum(X.fixed(x) ** 2 * c for x, c in zip(samples, counts))
    want = X.expected(n, S, Q)
    norm = X.normalised(lanes)
    assert X.S_Q_of(norm) == (S, Q) and X.in_headroom(norm)
    assert all(v <= X.M32 for k, v in enumerate(norm) if k not in (2, 7))
    for name, ln in (("canonical", lanes), ("normalised", norm)):
        got = host_finalize(fx, ln, n)
        assert same_float(got[0], want[0]), (name, "mean", got[0], want[0])
        assert same_float(got[1], want[1]), (name, "var", got[1], want[1])
    if n <= 4096:  # the header's own accumulation of the expanded list
        xs = np.repeat(np.asarray(samples, np.float64), counts)
        hl, m, v = host_lanes(fx, xs)
        assert hl == lanes
        assert same_float(m, want[0]) and same_float(v, want[1])


@pytest.mark.parametrize("name", list(CASES))
def test_reference_matches_the_host_header(fx, name):
    check_case(fx, *CASES[name])


@pytest.mark.parametrize("seed", range(200))
def test_reference_matches_the_host_header_on_random_mixes(fx, seed):
    check_case(fx, *random_case(seed))


def test_n_zero_and_below(fx):
    for n in (0, -3):
        got = host_finalize(fx, [0] * 8, n)
        want = X.expected(n, 0, 0)
        assert want[0] == 0.0 and np.isnan(want[1])
        assert bits(got[0]) == bits(0.0) and np.isnan(got[1])


def test_increments_are_the_headers(fx):
    """one sample at a time: the limb pieces of exact_ref.increments are fx_increments' words"""
    rng = np.random.default_rng(3)
    b = rng.integers(1, 1 << 16, 3000)
    a = rng.integers(0, 1 << 16, 3000)
    xs = list(X.samples_of(a, b)) + [0.0, 1.0, 93.0, 65535.0, q(1, 65535), q(65535, 65534), 2.0 ** -16, 4096.0]
    for x in xs:
        hl, _, _ = host_lanes(fx, [x])
        assert hl == X.increments(x), x


def small_shard(seed=9, n=600):
    rng = np.random.default_rng(seed)
    ent = np.sort(rng.integers(0, 12, n))
    glen = rng.integers(0, 700, n)
    arrays = {
        "uy_len": rng.choice([0, 1, 10, 31, 32, 255], n), "uy_gt30": rng.integers(0, 40, n),
        "cy_len": rng.choice([0, 16, 40], n), "cy_gt30": rng.integers(0, 17, n),
        "gq_len": glen, "gq_gt30": rng.integers(0, glen + 1), "gq_sum": rng.integers(0, 1 << 16, n),
    }
    return arrays, ent


def test_grouped_sums_match_a_per_record_fraction_loop():
    arrays, ent = small_shard()
    run, n_runs = X.runs_of(ent)
    a = X.sums_of(arrays, run, n_runs)
    b = X.naive_sums_of(arrays, run, n_runs)
    assert a.n == b.n and a.S == b.S and a.Q == b.Q
    # grouped by id, with ids that have no record
    a = X.sums_of(arrays, ent, 20, streams=3)
    b = X.naive_sums_of(arrays, ent, 20, streams=3)
    assert a.n == b.n and a.S == b.S and a.Q == b.Q
    assert a.n[15] == 0 and all(q == 0 for q in a.Q[15])
    mean, var = a.floats(cell=False)
    assert mean[15].tolist() == [0.0] * 4 and np.isnan(var[15, :3]).all() and var[15, 3] == 0.0


def test_floats_match_the_mean_and_variance_of_fractions():
    """expected() against the textbook formulas on the samples themselves (no 2^68 scaling)"""
    from fractions import Fraction

    arrays, ent = small_shard(seed=10, n=300)
    run, n_runs = X.runs_of(ent)
    s = X.sums_of(arrays, run, n_runs)
    mean, var = s.floats(cell=True)
    for e in range(n_runs):
        idx = np.flatnonzero(run == e)
        for st in range(4):
            num, den = X.STREAMS[st]
            xs = [Fraction(float(v)) for v in X.samples_of(arrays[num][idx], arrays[den][idx])]
            m = sum(xs) / len(xs)
            assert mean[e, st] == float(m)
            if len(xs) > 1:
                assert var[e, st] == float(sum((x - m) ** 2 for x in xs) / (len(xs) - 1))
            else:
                assert np.isnan(var[e, st])


def test_runs_of():
    run, k = X.runs_of(np.array([5, 5, 2, 2, 2, 5, 9]))
    assert run.tolist() == [0, 0, 1, 1, 1, 2, 3] and k == 4
