"""
Generate the FASTQ fixtures under tests/golden/fastq/ by running the UNMODIFIED reference
(``sctools.fastq``) where it is checked out.  No test imports this file.

    PYTHONDONTWRITEBYTECODE=1 python tools/make_fastq_golden.py REFERENCE_SRC

(``REFERENCE_SRC`` is the reference checkout's ``src`` directory, the one that holds ``sctools/``.)

What it writes (all data, no reference source):
* ``test_r1.fastq``, ``test_i7.fastq``, ``test_r1.fastq.gz``, ``test_r1.fastq.bz2``, ``test_r2.bam``
  copies of the reference's test inputs;
* ``expected_tags.json.gz``  per case, per generator, per record, the ``[tag, value]`` pairs the reference's
  ``EmbeddedBarcodeGenerator`` / ``BarcodeGeneratorWithCorrectedCellBarcodes`` yield:
  ``10x`` and ``10x_whitelist`` (the generators of ``TenXV2._make_tag_generators`` on r1 and i7, without and
  with ``1k-august-2016.txt``), ``10x_gz`` / ``10x_bz2`` (the r1 generator on the compressed copies) and
  ``attach_barcodes`` (the generators ``BarcodePlatform._make_tag_generators`` builds for the arguments of
  the reference's ``test_AttachBarcodes_entrypoint_with_whitelist``: a 7-base molecule barcode, sample
  barcode first);
* ``MANIFEST.json``          sha256 of each file.

``sctools.fastq`` needs ``pysam`` only through ``sctools.barcode``'s import; the stand-in ``pysam``
under ``tests/golden/stubs`` makes it importable.
"""
import gzip
import hashlib
import json
import os
import shutil
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "fastq")
if len(sys.argv) != 2:
    sys.exit(__doc__)
REF_SRC = sys.argv[1]
DATA = os.path.join(REF_SRC, "sctools", "test", "data")

sys.dont_write_bytecode = True
sys.path.insert(0, os.path.join(ROOT, "tests", "golden", "stubs"))
sys.path.insert(0, ROOT)  # the stub pysam reads BAMs with sctools_amd.bam
sys.path.insert(0, REF_SRC)

from sctools import consts, fastq  # noqa: E402

COPIES = ["test_r1.fastq", "test_i7.fastq", "test_r1.fastq.gz", "test_r1.fastq.bz2", "test_r2.bam"]
WHITELIST = os.path.join(DATA, "1k-august-2016.txt")

CELL = fastq.EmbeddedBarcode(start=0, end=16, quality_tag=consts.QUALITY_CELL_BARCODE_TAG_KEY,
                             sequence_tag=consts.RAW_CELL_BARCODE_TAG_KEY)
MOLECULE = fastq.EmbeddedBarcode(start=16, end=26, quality_tag=consts.QUALITY_MOLECULE_BARCODE_TAG_KEY,
                                 sequence_tag=consts.RAW_MOLECULE_BARCODE_TAG_KEY)
MOLECULE7 = MOLECULE._replace(end=23)
SAMPLE = fastq.EmbeddedBarcode(start=0, end=8, quality_tag=consts.QUALITY_SAMPLE_BARCODE_TAG_KEY,
                               sequence_tag=consts.RAW_SAMPLE_BARCODE_TAG_KEY)


def yields(generator):
    return [[[tag, value] for tag, value, kind in tag_set if kind == "Z"] for tag_set in generator]


def main():
    os.makedirs(OUT, exist_ok=True)
    for name in COPIES:
        shutil.copyfile(os.path.join(DATA, name), os.path.join(OUT, name))
        os.chmod(os.path.join(OUT, name), 0o644)
    r1, i7 = os.path.join(DATA, "test_r1.fastq"), os.path.join(DATA, "test_i7.fastq")
    cases = {
        "10x": [fastq.EmbeddedBarcodeGenerator(fastq_files=r1, embedded_barcodes=[CELL, MOLECULE]),
                fastq.EmbeddedBarcodeGenerator(fastq_files=i7, embedded_barcodes=[SAMPLE])],
        "10x_whitelist": [fastq.BarcodeGeneratorWithCorrectedCellBarcodes(
            fastq_files=r1, embedded_cell_barcode=CELL, whitelist=WHITELIST, other_embedded_barcodes=[MOLECULE]),
            fastq.EmbeddedBarcodeGenerator(fastq_files=i7, embedded_barcodes=[SAMPLE])],
        "10x_gz": [fastq.EmbeddedBarcodeGenerator(fastq_files=r1 + ".gz", embedded_barcodes=[CELL, MOLECULE])],
        "10x_bz2": [fastq.EmbeddedBarcodeGenerator(fastq_files=r1 + ".bz2", embedded_barcodes=[CELL, MOLECULE])],
        # platform.py:974-1001 with --i1 and --whitelist given: the sample generator is built from the r1 arguments
        "attach_barcodes": [fastq.EmbeddedBarcodeGenerator(fastq_files=r1, embedded_barcodes=[SAMPLE]),
                            fastq.BarcodeGeneratorWithCorrectedCellBarcodes(
                                fastq_files=r1, whitelist=WHITELIST, embedded_cell_barcode=CELL,
                                other_embedded_barcodes=[MOLECULE7])],
    }
    expected = {case: [yields(g) for g in generators] for case, generators in cases.items()}
    for case, per_generator in expected.items():
        print(case, [len(g) for g in per_generator], "records;",
              sum(1 for tags in per_generator[-1] if any(t == "CB" for t, _ in tags)), "with CB in the last generator")
    with open(os.path.join(OUT, "expected_tags.json.gz"), "wb") as raw:  # (mtime 0: the same bytes on every run)
        with gzip.GzipFile(filename="", mode="wb", fileobj=raw, mtime=0) as f:
            f.write(json.dumps(expected, separators=(",", ":")).encode())
    manifest = {}
    for name in sorted(os.listdir(OUT)):
        if name != "MANIFEST.json":
            manifest[name] = hashlib.sha256(open(os.path.join(OUT, name), "rb").read()).hexdigest()
    with open(os.path.join(OUT, "MANIFEST.json"), "w") as f:
        json.dump({"reference": "fredlas/sctools (2025-02-28 snapshot)", "sha256": manifest}, f, indent=1, sort_keys=True)


if __name__ == "__main__":
    main()
