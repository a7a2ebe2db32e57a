"""The exact-sum float mode on the device, held to exact rational arithmetic bit for bit.

fixedpt.h states the contract: a stream sample is x = RN(a / b), X = x 2^68 is an integer, an entity
keeps S = sum X and Q = sum X^2 as int64 sums of 32-bit limbs, and the mean and variance are the
correctly rounded quotients of the exact rationals.  tests/exact_ref.py restates it with Python
integers (tests/test_exact_ref_cpu.py holds that reference to the host build of the header); here
every float the device reports equals the reference's bit pattern, NaNs sit in the same places, and
every partial row's lanes rebuild the reference's S, Q and n.  No comparison has a tolerance: a
wrong limb, a dropped carry or a last-bit misrounding fails, and the message names the entity, the
stream, got - want of S and Q, and the highest differing bit.

(a) k_finalize alone on partial rows crafted at the edges of the documented headroom;
(b) the lanes kernels, the gene reduce and both views on the shards of test_gpu_stream_lanes.py and
    test_gpu_buckets.py, on the default path and on the global-sort path;
(c) one shard whose operands take every branch that chooses how a sample becomes lanes, once inside
    the narrow gene payload's fields and once beyond them;
(d) a shard of runs whose streams are constant: the RUN modes report floats only, and a variance that
    must be exactly 0.0 shows a fault in any limb, also one far below a double's precision.
"""
import functools

import numpy as np
import pytest
import torch

import exact_ref as X
from test_gpu_buckets import craft
from test_gpu_stream_lanes import BOUNDARIES, N_GENE_IDS, N_UMI_IDS, T, shard

pytestmark = pytest.mark.gpu

N31 = (1 << 31) - 1
N22 = 1 << 22


@pytest.fixture(scope="module")
def eng():
    from sctools_amd import engine as E

    return E.get_engine("cuda:0")


# ---- comparisons (all equalities) ----
def fbits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def assert_floats(gf, mean, var, what, names=None):
    """the eight stream columns of float rows gf [rows, SCT_NF] against mean / var [rows, 4]; names: a label
    per row for the message"""
    assert gf.shape[0] == mean.shape[0], (what, gf.shape, mean.shape)
    for st in range(X.N_STREAMS):
        for kind, col, want in (("mean", X.MEAN_COL[st], mean[:, st]), ("var", X.VAR_COL[st], var[:, st])):
            got = gf[:, col]
            gn, wn = np.isnan(got), np.isnan(want)
            bad = (gn != wn) | (~gn & ~wn & (fbits(got) != fbits(want)))
            if bad.any():
                e = int(np.flatnonzero(bad)[0])
                diff = int(fbits(got)[e]) ^ int(fbits(want)[e])
                label = "%d" % e if names is None else "%d (%s)" % (e, names[e])
                pytest.fail("%s: entity %s stream %d %s: got %r (%s), want %r (%s), highest differing bit %d of the "
                            "double; %d of %d rows differ" % (
                                what, label, st, kind, got[e], float(got[e]).hex(), want[e], float(want[e]).hex(),
                                X.top_bit(diff), int(bad.sum()), len(bad)))


def rebuilt(P, st):
    """S and Q of stream st of every partial row, as object arrays of Python ints"""
    ln = P[:, X.P_FLOAT + 8 * st:X.P_FLOAT + 8 * st + 8].astype(object)
    S = ln[:, 0] + ln[:, 1] * (1 << 32) + ln[:, 2] * (1 << 64)
    Q = ln[:, 3] + ln[:, 4] * (1 << 32) + ln[:, 5] * (1 << 64) + ln[:, 6] * (1 << 96) + ln[:, 7] * (1 << 128)
    return S, Q


def assert_partials(P, sums, what):
    """grouped gene partial rows [n_gene_ids, SCT_NP] against the reference's n, S and Q per gene id"""
    assert P.shape == (sums.n_ent, X.NP_ROW), (what, P.shape)
    n = np.array(sums.n, dtype=np.int64)
    bad = P[:, X.P_N] != n
    assert not bad.any(), "%s: entity %d: n got %d, want %d" % (
        what, np.flatnonzero(bad)[0], P[np.flatnonzero(bad)[0], X.P_N], n[np.flatnonzero(bad)[0]])
    assert (P[:, X.P_FLOAT:] >= 0).all(), "%s: a lane left the int64 headroom" % what
    dead = n == 0
    assert not P[dead, X.P_FLOAT:].any(), "%s: a gene without records has lanes" % what
    cy = P[:, X.P_FLOAT + 24:X.P_FLOAT + 32]
    assert not cy.any(), "%s: entity %d: the CY lanes of a grouped partial are not zero" % (
        what, np.flatnonzero(cy.any(axis=1))[0])
    live = np.flatnonzero(~dead)
    for st in range(3):
        S, Q = rebuilt(P[live], st)
        wS = np.array([sums.S[e][st] for e in live], dtype=object)
        wQ = np.array([sums.Q[e][st] for e in live], dtype=object)
        bad = (S != wS) | (Q != wQ)
        if bad.any():
            k = int(np.flatnonzero(bad)[0])
            dS, dQ = int(S[k] - wS[k]), int(Q[k] - wQ[k])
            pytest.fail("%s: entity %d stream %d: S got - want = %d (highest differing bit %d), Q got - want = %d "
                        "(highest differing bit %d); n = %d; %d of %d live rows differ" % (
                            what, live[k], st, dS, X.top_bit(int(S[k]) ^ int(wS[k])), dQ,
                            X.top_bit(int(Q[k]) ^ int(wQ[k])), n[live[k]], int(bad.sum()), len(bad)))


# ---- (a) k_finalize on crafted partials ----
def crafted_rows():
    """[(name, n, [(samples, counts)] per stream)]"""
    q = lambda a, b: float(X.samples_of(a, b))  # noqa: E731
    same = lambda s, c: [(s, c)] * X.N_STREAMS  # noqa: E731
    rows = [
        ("n1", 1, same([q(3, 10)], [1])),
        ("n2", 2, same([q(3, 10), q(7, 9)], [1, 1])),
        ("n2_equal", 2, same([q(1, 3)], [2])),
        ("constant", 1000, same([q(9, 10)], [1000])),
        ("constant_third", 77777, same([q(1, 3)], [77777])),
        ("all_zero", 50, same([0.0], [50])),
        ("n0", 0, same([], [])),
        ("1_65535_alone", 1, same([q(1, 65535)], [1])),
        ("1_65535_many", 4096, same([q(1, 65535)], [4096])),
        ("65535_alone", 1, same([65535.0], [1])),
        ("65535_and_1_65535", 2, same([65535.0, q(1, 65535)], [1, 1])),
        ("65535_and_1_65535_n22", N22, same([65535.0, q(1, 65535)], [N22 // 2, N22 // 2])),
        ("65535_once_among_1_65535", N22, same([65535.0, q(1, 65535)], [1, N22 - 1])),
        ("n22_of_65535", N22, same([65535.0], [N22])),
        ("n31_of_93", N31, same([93.0], [N31])),
        ("n31_93_and_a_third", N31, same([93.0, q(1, 3)], [1 << 30, (1 << 30) - 1])),
        ("n31_one_1_65535_among_93", N31, same([q(1, 65535), 93.0], [1, N31 - 1])),
        ("n31_of_a_third", N31, same([q(1, 3)], [N31])),
        ("n31_streams_differ", N31, [([q(2, 3), 0.0], [N31 - 5, 5]),
                                     ([q(92, 93), q(1, 93)], [N31 // 2, N31 - N31 // 2]),
                                     ([q(3700, 98), q(2000, 99), 93.0], [N31 - 1000, 999, 1]),
                                     ([q(16, 16), q(15, 16)], [N31 - 1, 1])]),
    ]
    rng = np.random.default_rng(2024)
    for k in range(300):
        n = int(rng.integers(1, 5000)) if k % 4 else int(rng.integers(1, 4))
        per = []
        for st in range(X.N_STREAMS):
            parts = min(n, int(rng.integers(1, 13)))
            cuts = np.sort(rng.choice(np.arange(1, n), parts - 1, replace=False)) if parts > 1 else np.array([], int)
            counts = np.diff(np.concatenate(([0], cuts, [n])))
            b = rng.integers(0 if k % 7 == 0 else 1, 1 << 16, parts)
            a = rng.integers(0, b + 1) if (k + st) % 2 else rng.integers(0, 1 << 16, parts)
            per.append((X.samples_of(a, b).tolist(), counts.tolist()))
        rows.append(("random%d" % k, n, per))
    return rows


@functools.lru_cache(maxsize=None)
def crafted_partials():
    """(names, partial rows [rows, SCT_NP], mean and var [rows, 4]): every row with canonical lanes, then once
    more with carry-normalised lanes"""
    names, P, mean, var = [], [], [], []
    for norm in (False, True):
        for name, n, per in crafted_rows():
            p = [0] * X.NP_ROW
            p[X.P_N] = n
            m, v = [], []
            for st, (samples, counts) in enumerate(per):
                assert sum(counts) == n and 0 <= n < (1 << 31)
                # the documented headroom: n < 2^31 while x <= 93, x up to 65535 while n <= 2^22
                assert all(0.0 <= x <= (93.0 if n > N22 else 65535.0) for x in samples), name
                lanes = X.lanes_of(samples, counts)
                if norm:
                    lanes = X.normalised(lanes)
                assert X.in_headroom(lanes), name
                p[X.P_FLOAT + 8 * st:X.P_FLOAT + 8 * st + 8] = lanes
                e = X.expected(n, *X.S_Q_of(lanes))
                m.append(e[0])
                v.append(e[1])
            names.append(name + ("/normalised" if norm else ""))
            P.append(p)
            mean.append(m)
            var.append(v)
    return names, np.array(P, dtype=np.int64), np.array(mean), np.array(var)


@pytest.mark.parametrize("mode", ["cell", "gene_grouped"])
def test_finalize_of_crafted_partials(eng, mode):
    """k_finalize alone (fx_finalize on the device: the big-integer product, subtraction, division and
    rounding): one launch over every crafted row."""
    names, P, mean, var = crafted_partials()
    half = len(names) // 2
    assert fbits(mean[:half]).tolist() == fbits(mean[half:]).tolist()  # normalised lanes: the same S and Q
    if mode != "cell":
        mean, var = mean.copy(), var.copy()
        mean[:, 3] = 0.0
        var[:, 3] = 0.0
    gi, gf = eng.finalize_partials(torch.from_numpy(P).to(eng.device), mode)
    gi, gf = gi.cpu().numpy(), gf.cpu().numpy()
    assert np.array_equal(gi[:, 0], P[:, X.P_N])
    assert_floats(gf, mean, var, "finalize_partials(%s)" % mode, names)


# ---- (b), (c): the engine on shards ----
class Ref:
    """a shard and its reference sums: by runs of the view's entity column and, for a cell-sorted shard,
    by gene id (the grouped partials)"""

    def __init__(self, arrays, mito, n_cell_ids, n_gene_ids, n_umi_ids, views):
        self.arrays, self.mito, self.dims = arrays, mito, (n_cell_ids, n_gene_ids, n_umi_ids)
        self.runs, self.grouped = {}, None
        for view in views:
            run, n_runs = X.runs_of(arrays[view])
            s = X.sums_of(arrays, run, n_runs, X.N_STREAMS if view == "cell" else 3)
            self.runs[view] = (s,) + s.floats(cell=view == "cell")
        if "cell" in views:
            s = X.sums_of(arrays, arrays["gene"], n_gene_ids, 3)
            self.grouped = (s,) + s.floats(cell=False)


def check_shard(eng, ref, what):
    from sctools_amd import engine as E

    dims = E.Dims(*ref.dims)
    cols = E.to_device(ref.arrays, eng.device)
    gm = torch.from_numpy(ref.mito).to(eng.device)
    for view, (s, mean, var) in ref.runs.items():
        gi, gf = eng.compute(cols, view, dims, gm, gm, float_mode="exact")
        assert gi[:, 0].cpu().tolist() == s.n, "%s: compute(%s) n_reads" % (what, view)
        assert_floats(gf.cpu().numpy(), mean, var, "%s: compute(%s)" % (what, view))
    if ref.grouped is None:
        return
    s, mean, var = ref.runs["cell"]
    ci, cf, part = eng.cell_and_gene(cols, dims, gm)
    assert ci[:, 0].cpu().tolist() == s.n, "%s: cell_and_gene n_reads" % what
    assert_floats(cf.cpu().numpy(), mean, var, "%s: cell_and_gene cell rows" % what)
    g, gmean, gvar = ref.grouped
    dead = np.array(g.n) == 0
    assert (gmean[dead] == 0.0).all() and np.isnan(gvar[dead, :3]).all() and (gvar[:, 3] == 0.0).all()
    for name, p in (("cell_and_gene", part), ("gene_partials", eng.gene_partials(cols, dims))):
        assert_partials(p.cpu().numpy(), g, "%s: %s partials" % (what, name))
        fi, ff = eng.finalize_partials(p)
        assert fi[:, 0].cpu().tolist() == g.n
        assert_floats(ff.cpu().numpy(), gmean, gvar, "%s: finalize_partials(%s)" % (what, name))


@functools.lru_cache(maxsize=None)
def stream_shard(n, heads, seed, view):
    arrays, mito, nc = shard(n, list(heads), seed, view)
    return Ref(arrays, mito, nc, N_GENE_IDS, N_UMI_IDS, (view,))


@pytest.mark.parametrize("view", ["cell", "gene"])
@pytest.mark.parametrize("n", [1, 255, T - 1, T, T + 1, 3 * T + 17])
def test_single_run_sizes(eng, n, view):
    check_shard(eng, stream_shard(n, (), 100 + n, view), "shard(%d, %s)" % (n, view))


@pytest.mark.parametrize("view", ["cell", "gene"])
@pytest.mark.parametrize("name", list(BOUNDARIES))
def test_run_boundaries(eng, name, view):
    n, heads = BOUNDARIES[name]
    check_shard(eng, stream_shard(n, tuple(heads), 7, view), "%s(%s)" % (name, view))


CRAFTED = [(50, 100, 1), (30_000, 1 << 20, 2)]


@functools.lru_cache(maxsize=None)
def craft_shard(n_gene_ids, n_umi_ids, seed):
    """big buckets, giants and thousands of tiny entities, ~45 k records, cell-sorted; its gene column
    is unsorted, so the gene view's entities are thousands of short runs"""
    arrays, mito, n_cells = craft(n_gene_ids, n_umi_ids, seed)
    return Ref(arrays, mito, n_cells, n_gene_ids, n_umi_ids, ("cell", "gene"))


@pytest.mark.parametrize("path", ["buckets", "global_sort"])
@pytest.mark.parametrize("n_gene_ids,n_umi_ids,seed", CRAFTED)
def test_bucket_edge_cases(eng, monkeypatch, n_gene_ids, n_umi_ids, seed, path):
    if path == "global_sort":  # this path takes its samples in finalize.h
        monkeypatch.setenv("SCT_FORCE_GLOBAL_SORT", "1")
    what = "craft(%d, %d, %d) on %s" % (n_gene_ids, n_umi_ids, seed, path)
    check_shard(eng, craft_shard(n_gene_ids, n_umi_ids, seed), what)


# (c) operand edges: (numerator, denominator) pairs of the barcode streams and (gq_gt30, gq_len, gq_sum)
# triples of the genomic ones.  Narrow: every value inside the narrow gene payload's fields (uy 5 bits,
# gq_gt30 / gq_len 9 bits, gq_sum 15 bits); wide: beyond them too.
U8_NARROW = [(0, 1), (1, 1), (0, 10), (3, 10), (10, 10), (0, 31), (17, 31), (31, 31),  # table hits when B is the tile's
             (11, 10), (20, 10), (31, 1), (31, 30),  # a > B: the table guard fails, x > 1
             (5, 0), (31, 0), (0, 0)]  # a / 0 = 0
U8_WIDE = U8_NARROW + [(0, 32), (7, 32), (32, 32), (128, 255), (255, 255), (33, 32), (200, 10), (255, 1), (255, 0),
                       (32, 31)]
GQ_NARROW = [(g if g is not None else ln, ln, s) for ln in (0, 1, 255, 256, 511) for g in (0, 1, None, 511)
             for s in (0, 1, 32767)]
GQ_WIDE = [(g if g is not None else ln, ln, s) for ln in (0, 1, 255, 256, 511, 512, 65535)
           for g in (0, None, 511, 512, 65535) for s in (0, 1, 32767, 32768, 65535)]
N_EDGE = 2 * T + 100


@functools.lru_cache(maxsize=None)
def edge_shard(view, wide):
    arrays, mito, nc = shard(N_EDGE, [5000, T + 77], 61, view)
    arrays = {k: v.copy() for k, v in arrays.items()}
    rng = np.random.default_rng(62 + wide)
    # record 0 keeps uy_len 10, cy_len 16: tile 0 has both tables
    inner = np.setdiff1d(np.arange(1, N_EDGE), [T, 2 * T])

    def put(cols, cases, k):
        at = rng.choice(inner, k, replace=False)
        pick = np.array(cases)[np.arange(k) % len(cases)]
        for j, c in enumerate(cols):
            arrays[c][at] = pick[:, j]

    put(("uy_gt30", "uy_len"), U8_WIDE if wide else U8_NARROW, 2400)
    put(("cy_gt30", "cy_len"), U8_WIDE, 2400)  # cy is not in the gene payload
    put(("gq_gt30", "gq_len", "gq_sum"), GQ_WIDE if wide else GQ_NARROW, 3000)
    # tile 1's first record: no cy table and, wide, no uy table (40 >= 32); tile 2's: a zero denominator as the
    # tabulated one
    arrays["cy_len"][T], arrays["cy_gt30"][T] = 40, 33
    if wide:
        arrays["uy_len"][T], arrays["uy_gt30"][T] = 40, 33
    else:  # tile 1 tabulates B = 31
        arrays["uy_len"][T], arrays["uy_gt30"][T] = 31, 17
    arrays["uy_len"][2 * T], arrays["uy_gt30"][2 * T] = 0, 3
    arrays["cy_len"][2 * T], arrays["cy_gt30"][2 * T] = 0, 0
    for c in ("uy_gt30", "cy_gt30", "gq_gt30", "gq_sum"):  # stretches of all-zero numerators
        arrays[c][300:900] = 0
        arrays[c][T + 4000:T + 4100] = 0
    narrow = (arrays["uy_len"].max() < 32 and arrays["uy_gt30"].max() < 32 and arrays["gq_len"].max() < 512
              and arrays["gq_gt30"].max() < 512 and arrays["gq_sum"].max() < 32768)
    assert narrow == (not wide)
    for num, den in X.STREAMS:  # the branches the shard is for
        a, b = arrays[num].astype(int), arrays[den].astype(int)
        assert ((b == 0) & (a > 0)).any() and ((b == 0) & (a == 0)).any() and (a > b).any() and (a == b).any()
    return Ref(arrays, mito, nc, N_GENE_IDS, N_UMI_IDS, (view,))


@functools.lru_cache(maxsize=None)
def constant_runs_shard(view):
    """850 runs of 2 to 40 records over three tiles, every stream constant inside a run (the edge operands
    above, one tuple per run): S^2 = n Q exactly, so the variance is 0.0 and any fault in any limb of any
    lane, however far below a double's precision, leaves a non-zero or wrapped variance.  The RUN modes
    report floats only; this is what makes their low limbs visible."""
    rng = np.random.default_rng(71)
    lens = rng.integers(2, 41, 850)
    heads = np.cumsum(lens)[:-1]
    n = int(lens.sum())
    assert 2 * T < n < 3 * T
    arrays, mito, nc = shard(n, heads.tolist(), 72, view)
    arrays = {k: v.copy() for k, v in arrays.items()}
    run = np.repeat(np.arange(lens.size), lens)
    for cols, cases in ((("uy_gt30", "uy_len"), U8_WIDE), (("cy_gt30", "cy_len"), U8_WIDE),
                        (("gq_gt30", "gq_len", "gq_sum"), GQ_WIDE)):
        # every third run keeps the tabulated barcode length (uy 10, cy 16) with a numerator of its own
        pick = np.array(cases)[rng.integers(0, len(cases), lens.size)]
        if len(cols) == 2:
            base = 10 if cols[1] == "uy_len" else 16
            pick[::3, 1] = base
            pick[::3, 0] = rng.integers(0, base + 1, pick[::3].shape[0])
        for j, c in enumerate(cols):
            arrays[c][:] = pick[run, j]
    ref = Ref(arrays, mito, nc, N_GENE_IDS, N_UMI_IDS, (view,))
    var = ref.runs[view][2]
    assert (var == 0.0).all() and not np.signbit(var).any()
    return ref


@pytest.mark.parametrize("view", ["cell", "gene"])
def test_constant_runs_have_zero_variance(eng, view):
    check_shard(eng, constant_runs_shard(view), "constant runs (%s)" % view)


@pytest.mark.parametrize("view", ["cell", "gene"])
@pytest.mark.parametrize("wide", [False, True], ids=["narrow", "wide"])
def test_operand_edges(eng, view, wide):
    """Increment-table hits and misses, tiles without a table, rcp_of inside and outside its LDS table
    (gq_len 255 / 256), both gene payload formats (511 / 512, 32767 / 32768), x > 1, and zero
    denominators in every run: the reference defines a / 0 = 0, so no row is left out."""
    check_shard(eng, edge_shard(view, wide), "operand edges (%s, %s)" % (view, "wide" if wide else "narrow"))
