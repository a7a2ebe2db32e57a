"""
Generate the barcode fixtures under tests/golden/barcode/ by running the UNMODIFIED reference
(``sctools.barcode``, ``sctools.encodings``) in the build container.

Run here only (the reference never leaves this container):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_barcode_golden.py REFERENCE_SRC

(``REFERENCE_SRC`` is the reference checkout's ``src`` directory, the one that holds ``sctools/``.)

What it writes (all data, no reference source):
* ``1k-august-2016.txt``        a copy of the reference's bundled whitelist (1001 16-mers);
* ``crafted_L8.txt``            ~100 8-mers with distance-1 pairs, chains a-b-c and duplicate lines, shuffled;
* ``crafted_L5_nonewline.txt``  5-mers, the last line unterminated (it loses its last base on reading);
* ``crafted_L21.txt``           21-mers, the same shapes;
* ``corrections.json.gz``         per whitelist, ``[query, corrected-or-null]`` from the reference's own
  ``ErrorsToCorrectBarcodesMap``: every key of the crafted maps; for the 1k list every whitelist
  barcode, 2000 single-base errors (``N`` included), 500 double errors, lower case, ``NN...``, wrong
  lengths and the empty string;
* ``pair_stats.json``           per whitelist, the reference's ``summarize_hamming_distances()``,
  ``base_frequency()`` and ``effective_diversity()`` (floats as ``repr``), and ``TwoBit`` samples;
* ``MANIFEST.json``             sha256 of each file.

The stand-in ``pysam`` under ``tests/golden/stubs`` makes the reference importable.
"""
import gzip
import hashlib
import json
import os
import random
import shutil
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "barcode")
if len(sys.argv) != 2:
    sys.exit(__doc__)
REF_SRC = sys.argv[1]

sys.dont_write_bytecode = True
sys.path.insert(0, os.path.join(HERE, "stubs"))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))  # the stub pysam reads BAMs with sctools_amd.bam
sys.path.insert(0, REF_SRC)

from sctools.barcode import Barcodes, ErrorsToCorrectBarcodesMap  # noqa: E402
from sctools.encodings import TwoBit  # noqa: E402

LENGTHS = {"1k-august-2016.txt": 16, "crafted_L8.txt": 8, "crafted_L5_nonewline.txt": 5, "crafted_L21.txt": 21}


def substitute(rng, barcode, alphabet="ACGT", avoid=()):
    while True:
        pos = rng.randrange(len(barcode))
        if pos in avoid:
            continue
        base = rng.choice([b for b in alphabet if b != barcode[pos]])
        return barcode[:pos] + base + barcode[pos + 1:], pos


def crafted(rng, length, n_seeds):
    """Seeds; a distance-1 neighbour for half of them; a third link for a quarter (a chain a-b-c, c at
    distance 2 from a); duplicate lines; shuffled, so that the largest file index is not the last made."""
    out = []
    for k in range(n_seeds):
        a = "".join(rng.choice("ACGT") for _ in range(length))
        out.append(a)
        if k % 2 == 0:
            b, pos = substitute(rng, a)
            out.append(b)
            if k % 4 == 0 and length > 1:
                out.append(substitute(rng, b, avoid=(pos,))[0])
        if k % 5 == 0:
            out.append(a)
        if k % 7 == 0:  # a second neighbour of a at the same position: a, b, b' pairwise at distance 1
            out.append(substitute(rng, a)[0])
    rng.shuffle(out)
    return out


def corrections(ref_map, queries):
    return [[q, ref_map._map.get(q)] for q in queries]


def main():
    os.makedirs(OUT, exist_ok=True)
    rng = random.Random(20160801)
    shutil.copyfile(os.path.join(REF_SRC, "sctools", "test", "data", "1k-august-2016.txt"),
                    os.path.join(OUT, "1k-august-2016.txt"))
    with open(os.path.join(OUT, "crafted_L8.txt"), "w") as f:
        f.write("".join(b + "\n" for b in crafted(rng, 8, 48)))
    with open(os.path.join(OUT, "crafted_L5_nonewline.txt"), "w") as f:
        f.write("\n".join(crafted(rng, 5, 12)))  # no newline after the last line
    with open(os.path.join(OUT, "crafted_L21.txt"), "w") as f:
        f.write("".join(b + "\n" for b in crafted(rng, 21, 24)))

    fixed = {}
    stats = {}
    for name, length in LENGTHS.items():
        path = os.path.join(OUT, name)
        ref_map = ErrorsToCorrectBarcodesMap.single_hamming_errors_from_whitelist(path)
        lines = [line[:-1] for line in open(path)]
        if name.startswith("crafted"):
            queries = list(ref_map._map)  # every key
            queries += [q.lower() for q in lines[:5]] + ["N" * length, "NN" + lines[0][2:], "", lines[0][:-1],
                                                          lines[0] + "A"]
            queries += [substitute(rng, substitute(rng, q)[0])[0] for q in lines]  # double errors (some fold back)
            queries += [substitute(rng, q, "ACGTN")[0] for q in lines for _ in range(3)]
        else:
            queries = list(lines)
            queries += [substitute(rng, rng.choice(lines), "ACGTN")[0] for _ in range(2000)]
            for _ in range(500):
                q, pos = substitute(rng, rng.choice(lines), "ACGTN")
                queries.append(substitute(rng, q, "ACGTN", avoid=(pos,))[0])
            queries += [q.lower() for q in lines[:20]] + [q[:8] + q[8:].lower() for q in lines[20:30]]
            queries += ["N" * length, "NN" + lines[0][2:], lines[1][:7] + "NN" + lines[1][9:], "", "A", lines[0][:-1],
                        lines[0] + "A", lines[0] + lines[1], lines[2][:15] + "X", lines[3][:15] + "-"]
        fixed[name] = corrections(ref_map, queries)

        random.seed(2016)  # TwoBit draws a base for an ambiguity code (the 1k list's last line starts with N)
        barcodes = Barcodes.from_whitelist(path, length)
        summary = barcodes.summarize_hamming_distances()
        coder = TwoBit(length)
        keys = list(barcodes)
        stats[name] = {
            "barcode_length": length,
            "n_barcodes": len(barcodes),
            "summarize_hamming_distances": {k: repr(float(v)) for k, v in summary.items()},
            "base_frequency": [[int(c) for c in row] for row in barcodes.base_frequency()],
            "effective_diversity": [repr(float(v)) for v in barcodes.effective_diversity()],
            # [barcode, code, decode(code), gc_content(code)] for lines of the file's length
            "twobit": [[b, TwoBit.encode(b.encode()), coder.decode(TwoBit.encode(b.encode())).decode(),
                        coder.gc_content(TwoBit.encode(b.encode()))] for b in lines[:12] if len(b) == length],
            # [code a, code b, hamming_distance(a, b)]
            "hamming": [[a, b, TwoBit.hamming_distance(a, b)]
                        for a, b in (rng.sample(keys, 2) for _ in range(20))],
        }
        print(name, len(lines), "lines,", len(fixed[name]), "queries,",
              sum(1 for q, c in fixed[name] if c is not None), "corrected,",
              sum(1 for q, c in fixed[name] if c is not None and q in lines and c != q), "whitelist entries moved")

    with open(os.path.join(OUT, "corrections.json.gz"), "wb") as raw:  # (mtime 0: the same bytes on every run)
        with gzip.GzipFile(filename="", mode="wb", fileobj=raw, mtime=0) as f:
            f.write(json.dumps(fixed, separators=(",", ":")).encode())
    with open(os.path.join(OUT, "pair_stats.json"), "w") as f:
        f.write("{\n" + ",\n".join("%s: %s" % (json.dumps(k), json.dumps(v, sort_keys=True, separators=(",", ":")))
                                   for k, v in sorted(stats.items())) + "\n}\n")
    manifest = {}
    for name in sorted(os.listdir(OUT)):
        if name != "MANIFEST.json":
            manifest[name] = hashlib.sha256(open(os.path.join(OUT, name), "rb").read()).hexdigest()
    with open(os.path.join(OUT, "MANIFEST.json"), "w") as f:
        json.dump({"reference": "fredlas/sctools (2025-02-28 snapshot)", "sha256": manifest}, f, indent=1, sort_keys=True)


if __name__ == "__main__":
    main()
