"""The per-entity width of the first partition level (bucket.h l1_width) and the run structure
published once per step (segment.h: head bitmap, k_ent_starts) against the oracle.

One crafted shard holds cell runs at every size where the level-1 digit width changes, a run that is
an inner slot of its key tile, a level 2 below a narrow level 1, a giant, a recurring cell id and a
partial last tile.  SCT_L1_BITS=8 (the uniform width of earlier rounds) must give the same rows.
"""
import os
import re

import numpy as np
import pytest
import torch

from oracle import oracle as O

pytestmark = pytest.mark.gpu

REL = 1e-9
N_GENES, N_UMIS = 30_000, 1 << 20
K_BIG_CAP = 3071   # bucket.h kBigCap: a larger run is a level-1 segment
K_RADIX_BITS = 8
K_KTILE = 8192     # segment.h kKTile


def _header_const(name):
    src = open(os.path.join(os.path.dirname(__file__), "..", "sctools_amd", "csrc", "bucket.h")).read()
    m = re.search(r"#define %s (\d+)" % name, src) or re.search(r"constexpr int %s = (\d+);" % name, src)
    assert m, name
    return int(m.group(1))


K_L1_TARGET = _header_const("SCT_L1_TARGET")
K_L1_MIN_BITS = _header_const("kL1MinBits")


def l1_width(size):
    """bucket.h l1_width: clamp(ceil_log2(ceil(size / kL1Target)), kL1MinBits, kRadixBits)."""
    q = -(-size // K_L1_TARGET)
    return min(max((q - 1).bit_length(), K_L1_MIN_BITS), K_RADIX_BITS)


def columns(cell, gene, umi, ref, pos, unmapped, rng, plus_strand=None):
    n = len(cell)
    unm = np.asarray(unmapped, bool)
    bits = np.where(unm, 1, 0) | np.where(rng.random(n) < 0.5, 2, 0)
    if plus_strand is not None:
        bits[plus_strand] &= ~2
    bits |= np.where(~unm & (rng.random(n) < 0.3), 4, 0) | np.where(~unm & (rng.random(n) < 0.1), 8, 0)
    bits |= np.where(~unm & (rng.random(n) < 0.8), 16, 0) | np.where(rng.random(n) < 0.9, 32, 0)
    bits |= 64 | np.where(rng.random(n) < 0.95, 128, 0)
    glen = rng.integers(30, 99, n)
    return {
        "cell": np.asarray(cell, np.int32), "umi": np.asarray(umi, np.int32), "gene": np.asarray(gene, np.int32),
        "ref": np.where(unm, -1, ref).astype(np.int32), "pos": np.where(unm, -1, pos).astype(np.int32),
        "gq_len": glen.astype(np.uint16), "gq_sum": (glen * rng.integers(20, 40, n)).astype(np.uint16),
        "gq_gt30": rng.integers(0, glen + 1).astype(np.uint16), "bits": bits.astype(np.uint8),
        "xf": np.where(unm, 0, rng.integers(1, 5, n)).astype(np.uint8),
        "cy_len": np.full(n, 16, np.uint8), "cy_gt30": rng.integers(0, 17, n).astype(np.uint8),
        "uy_len": np.full(n, 10, np.uint8), "uy_gt30": rng.integers(0, 11, n).astype(np.uint8),
    }


def background(size, rng):
    """`size` records of one run: Zipf-like genes, random molecules, 3 % unmapped."""
    gene = np.minimum((N_GENES * rng.random(size) ** 3).astype(np.int64), N_GENES - 1)
    return (gene, rng.integers(0, N_UMIS, size), rng.integers(0, 25, size), rng.integers(0, 1 << 20, size),
            rng.random(size) < 0.03)


def run_sizes():
    """The crafted shard's run sizes in input order, and the indices of the special runs."""
    edges = []
    k = 0
    while True:
        s = K_L1_TARGET << k
        if s + 1 > K_BIG_CAP and l1_width(s) != l1_width(s + 1):
            edges.append(s)
        if l1_width(s + 1) >= K_RADIX_BITS:
            break
        k += 1
    sizes = [K_BIG_CAP, K_BIG_CAP + 2, K_BIG_CAP + 1]  # tile 0: first run, an inner slot, the last run
    for s in edges:
        for x in (s - 1, s, s + 1):
            if x not in sizes:
                sizes.append(x)
    sizes.append(57)  # the first run's cell id again, not adjacent to it
    return sizes


@pytest.fixture(scope="module")
def shard():
    rng = np.random.default_rng(7)
    sizes = run_sizes()
    n = sum(sizes)
    assert n <= 300_000 and n % K_KTILE != 0, n
    starts = np.concatenate(([0], np.cumsum(sizes)))
    # the second run lies inside key tile 0, between two other runs: an inner slot
    assert starts[1] > 0 and starts[2] < K_KTILE and sizes[1] > K_BIG_CAP
    widths = {l1_width(s) for s in sizes if s > K_BIG_CAP}
    assert len(widths) >= 3 and K_RADIX_BITS in widths, widths
    # a run over >= 3 key tiles with a narrow level 1 whose hottest gene needs a level 2; a run with a giant
    deep = next(i for i, s in enumerate(sizes) if s > 2 * K_KTILE + 2 and l1_width(s) < K_RADIX_BITS)
    assert starts[deep] // K_KTILE + 2 <= (starts[deep + 1] - 1) // K_KTILE
    giant = next(i for i, s in enumerate(sizes) if s > 4 * K_BIG_CAP and i != deep)
    cols = [[] for _ in range(5)]
    cell, plus = [], []
    for i, size in enumerate(sizes):
        g, u, r, p, unm = background(size, rng)
        ps = np.zeros(size, bool)
        if i == deep:  # one gene with 4000 records over many UMIs
            g[:4000], unm[:4000] = 17, False
        if i == giant:  # one molecule at one fragment
            m = K_BIG_CAP + 130
            g[:m], u[:m], r[:m], p[:m], unm[:m], ps[:m] = 23, 5, 3, 777, False, True
        perm = rng.permutation(size)  # input order inside an entity is arbitrary
        for dst, src in zip(cols, (g, u, r, p, unm)):
            dst.append(src[perm])
        plus.append(ps[perm])
        cell.append(np.full(size, 0 if i == len(sizes) - 1 else i, np.int64))
    gene, umi, ref, pos, unm = (np.concatenate(c) for c in cols)
    arrays = columns(np.concatenate(cell), gene, umi, ref, pos, unm, rng, np.concatenate(plus))
    mito = np.zeros(N_GENES, np.uint8)
    mito[[17, 40]] = 1
    n_sorted = n - sizes[-1]  # without the recurring cell id: valid input for the grouped gene view
    want = {"cell": O.run(arrays, "cell", mito, N_GENES, threads=8)}
    head = {c: a[:n_sorted] for c, a in arrays.items()}
    want["cell_sorted"] = O.run(head, "cell", mito, N_GENES, threads=8)
    want["grouped"] = O.run(head, "gene_grouped", mito, N_GENES, threads=8)
    return {"arrays": arrays, "mito": mito, "n_cells": len(sizes), "n_runs": len(sizes), "n_sorted": n_sorted,
            "want": want}


@pytest.fixture(scope="module")
def eng():
    from sctools_amd import engine as E

    return E.get_engine("cuda:0")


def compare(gi, gf, oi, of, exact):
    """tests/test_gpu_buckets.py's rule: integers exactly; Welford floats exactly, exact-sum floats to 1e-9."""
    assert gi.shape == oi.shape
    assert np.array_equal(gi, oi), np.argwhere(gi != oi)[:10]
    ng, no = np.isnan(gf), np.isnan(of)
    assert np.array_equal(ng, no)
    if exact:
        assert np.array_equal(gf[~ng], of[~no])
    else:
        x, y = gf[~ng], of[~no]
        rel = np.abs(x - y) / np.maximum(np.maximum(np.abs(x), np.abs(y)), 1e-300)
        assert (rel <= REL).all(), rel.max()


def rows_of(eng, shard):
    from sctools_amd import engine as E

    dims = E.Dims(shard["n_cells"], N_GENES, N_UMIS)
    gm = torch.from_numpy(shard["mito"]).to(eng.device)
    cols = E.to_device(shard["arrays"], eng.device)
    out = {}
    for fm in ("welford", "exact"):
        gi, gf = eng.compute(cols, "cell", dims, gm, gm, float_mode=fm)
        out[fm] = (gi.cpu().numpy(), gf.cpu().numpy())
    head = {c: t[:shard["n_sorted"]] for c, t in cols.items()}
    ci, cf, part = eng.cell_and_gene(head, dims, gm)
    gi, gf = eng.finalize_partials(part)
    out["combined_cell"] = (ci.cpu().numpy(), cf.cpu().numpy())
    out["grouped"] = (gi.cpu().numpy(), gf.cpu().numpy())
    return out


def check_rows(got, shard):
    want = shard["want"]
    assert got["welford"][0].shape[0] == shard["n_runs"]
    compare(*got["welford"], *want["cell"], exact=True)
    compare(*got["exact"], *want["cell"], exact=False)
    compare(*got["combined_cell"], *want["cell_sorted"], exact=False)
    oi, of = want["grouped"]
    gi, gf = got["grouped"]
    live = oi[:, 0] > 0
    assert np.array_equal(gi[:, 0] > 0, live)
    compare(gi[live], gf[live], oi[live], of[live], exact=False)


def test_every_level1_width_matches_the_oracle(eng, shard, monkeypatch):
    monkeypatch.delenv("SCT_L1_BITS", raising=False)
    check_rows(rows_of(eng, shard), shard)


def test_uniform_width_switch_gives_identical_rows(eng, shard, monkeypatch):
    monkeypatch.delenv("SCT_L1_BITS", raising=False)
    a = rows_of(eng, shard)
    monkeypatch.setenv("SCT_L1_BITS", "8")
    b = rows_of(eng, shard)
    check_rows(b, shard)
    for k in a:
        assert np.array_equal(a[k][0], b[k][0]), k
        assert np.array_equal(np.nan_to_num(a[k][1], nan=7.0).view(np.int64),
                              np.nan_to_num(b[k][1], nan=7.0).view(np.int64)), k


@pytest.mark.parametrize("n,shift", [(1, 0), (8191, 0), (8193, 0), (8193, 1), (1, 1)])
def test_run_structure_edges(eng, n, shift):
    """The head bitmap and the entity starts at tile edges (one record, one short of and one past a key
    tile) and for an entity column that is not 16-byte aligned (k_heads instead of k_heads4)."""
    from sctools_amd import engine as E

    rng = np.random.default_rng(100 + n)
    sizes, left = [], n
    for s in (3500, 1, 63, 3200, 2, 64, 700):  # segments, word-sized runs, a run over the tile edge
        s = min(s, left)
        if s:
            sizes.append(s)
        left -= s
    if left:
        sizes.append(left)
    parts = [background(s, rng) for s in sizes]
    gene, umi, ref, pos, unm = (np.concatenate([p[i] for p in parts]) for i in range(5))
    cell = np.repeat((np.arange(len(sizes)) * 5 + 2) % 11, sizes)  # ids recur, never in adjacent runs
    arrays = columns(cell, gene, umi, ref, pos, unm, rng)
    mito = np.zeros(N_GENES, np.uint8)
    mito[40] = 1
    dims = E.Dims(11, N_GENES, N_UMIS)
    gm = torch.from_numpy(mito).to(eng.device)
    cols = E.to_device(arrays, eng.device)
    buf = torch.zeros(n + 4, dtype=torch.int32, device=eng.device)
    off = (-buf.data_ptr() // 4) % 4 + shift  # int32 elements to the next 16-byte boundary, plus the shift
    buf[off:off + n] = cols["cell"]
    cols["cell"] = buf[off:off + n]
    assert (cols["cell"].data_ptr() % 16 == 0) == (shift == 0)
    oi, of = O.run(arrays, "cell", mito, N_GENES, threads=8)
    assert oi.shape[0] == len(sizes)
    for fm in ("welford", "exact"):
        gi, gf = eng.compute(cols, "cell", dims, gm, gm, float_mode=fm)
        compare(gi.cpu().numpy(), gf.cpu().numpy(), oi, of, exact=fm == "welford")
