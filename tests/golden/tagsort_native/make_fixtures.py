"""
Regenerates the fixtures of this directory: for every case the reads as columns (``<case>.json``),
the 17-field lines the reference's per-read stage would write for them (``<case>.lines.txt``), and
the metrics CSVs the REFERENCE's gatherer writes from those lines (``<case>.cell.csv``,
``<case>.gene.csv``).

The gatherer (``metricgatherer.cpp``, ``mitochondrial_gene_selector.cpp``, ``utilities.cpp`` of the
reference's ``fastqpreprocessing/src``) compiles without htslib.  This script builds it with the small
driver below into a temporary directory, feeds it each case's lines and records what it writes.
Nothing of the reference is kept.  Usage::

    python tests/golden/tagsort_native/make_fixtures.py /path/to/reference/fastqpreprocessing/src

Every case is built so that its result does not depend on the order of equal triplets (the reference
leaves that order undefined); the script checks it by shuffling equal triplets.
"""
import json
import os
import random
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [TESTS, os.path.dirname(TESTS)]
import tagsort_ref as R  # noqa: E402

DRIVER = r"""
#include <fstream>
#include <memory>
#include <string>
#include "metricgatherer.h"
// driver <cell|gene> <lines> <csv> [<gtf> <names>]: what tagsort.cpp does around the gatherer
int main(int argc, char** argv) {
  const std::string type = argv[1];
  std::unique_ptr<MetricGatherer> g;
  if (type == "cell") g = std::make_unique<CellMetricGatherer>(argv[4], argv[5]);
  else g = std::make_unique<GeneMetricGatherer>();
  g->clear();
  std::ofstream out(argv[3]);
  out << g->getHeader() << std::endl;
  std::ifstream in(argv[2]);
  for (std::string line; std::getline(in, line);) g->ingestLine(line, out);
  g->output_metrics(out);
  g->output_metrics_extra(out);
  return 0;
}
"""

GTF = "\n".join([
    "#!genome-build fixture",
    'chrM\tfix\tgene\t1\t100\t.\t+\t.\tgene_id "ENSG_MT1"; gene_name "mt-Co1";',
    'chrM\tfix\tgene\t200\t300\t.\t+\t.\tgene_id "G2"; gene_name "MT-ND1";',
    'chrM\tfix\ttranscript\t200\t300\t.\t+\t.\tgene_id "G2"; transcript_id "T2"; gene_name "MT-ND1";',
    'chr1\tfix\tgene\t1\t100\t.\t+\t.\tgene_id "G3"; gene_name "Actb";',
    'chr1\tfix\tgene\t500\t900\t.\t-\t.\tgene_id "GX"; gene_name "Special";',
    ""])
NAMES = "# names counted as mitochondrial\n\nmt-Co1\nSpecial\n"


def rd(first, second, third, ref="chr1", pos=100, strand=0, xf="CODING", nh=1, cy=(14, 16), uy=(9, 10),
       gq=(3000, 98, 90), perfect_umi=1, perfect_cb=1, dup=0, spliced=0):
    return dict(first=first, second=second, third=third, ref=ref, xf=xf, pos=pos, strand=strand, cy_gt30=cy[0],
                cy_len=cy[1], gq_sum=gq[0], gq_len=gq[1], gq_gt30=gq[2], nh=nh, perfect_umi=perfect_umi,
                spliced=spliced, dup=dup, perfect_cb=perfect_cb, uy_gt30=uy[0], uy_len=uy[1])


def un(first, second, third, **kw):
    kw.setdefault("xf", "")
    kw.setdefault("nh", -1)
    return rd(first, second, third, ref="*", pos=0, **kw)


def cases():
    c = {}
    c["leading_unmapped"] = [
        un("A", "AAA", "G1"), un("A", "AAC", "G1", uy=(3, 10)), un("B", "AAA", "G2", cy=(1, 16)),
        un("C", "AAA", "G1"), rd("C", "CCC", "G1", uy=(10, 10)), rd("C", "GGG", "G3", xf="INTRONIC", gq=(2000, 98, 40)),
        rd("D", "AAA", "G1", xf="UTR"), rd("D", "AAC", "G1", nh=3, dup=1)]
    c["unmapped_starts"] = [
        rd("A", "CCC", "G1"), rd("A", "CCG", "G2", uy=(5, 10)),
        un("B", "AAA", "G1"), rd("B", "CCC", "G1"), rd("B", "CCG", "G1", spliced=1),
        un("C", "AAA", "G1", uy=(2, 10)), un("C", "AAC", "G1"), rd("C", "CCC", "G2", xf="INTERGENIC"),
        un("D", "AAA", "G1"), un("D", "AAC", "G2", cy=(0, 16)), un("D", "AAG", "G2"), rd("D", "CCC", "G1"),
        rd("D", "CCG", "G1", pos=500, strand=1)]
    c["no_mapped_between"] = [
        rd("A", "AAA", "G1"), un("B", "AAA", "G1"), un("B", "AAC", "G2", uy=(1, 10)),
        rd("C", "AAA", "G1", perfect_cb=0), rd("C", "AAC", "G1", perfect_umi=0)]
    c["last_unmapped"] = [
        rd("A", "AAA", "G1"), rd("A", "AAC", "G1", gq=(2500, 98, 70)), rd("B", "AAA", "G2"),
        un("B", "TTT", "G9", uy=(4, 10), xf="INTERGENIC")]
    c["none_tags"] = [
        rd("Mcell", "AAA", "G1"), rd("Mcell", "None", "G1", uy=(0, 0), perfect_umi=0),
        rd("Mcell", "CCC", "None", xf="", uy=(6, 10)),
        rd("None", "AAA", "G1", perfect_cb=0), un("None", "AAC", "G1", perfect_cb=0),
        rd("None", "None", "None", perfect_cb=0, xf=""),
        un("Ocell", "AAA", "None"), rd("Ocell", "None", "None", xf="", pos=7), rd("Ocell", "TTT", "G1")]
    c["multi_gene"] = [
        rd("G1", "CellA", "AAA"), rd("G1", "CellB", "AAA", uy=(7, 10)),
        rd("G1,G2", "CellA", "AAA"), rd("G1,G2", "CellA", "AAC", pos=300), un("G1,G2", "CellC", "AAA"),
        un("G3", "CellA", "AAA"), rd("G3", "CellA", "AAC"), rd("G3", "CellB", "AAA", cy=(16, 16))]
    c["all_dropped"] = [rd("None", "AAA", "G1"), un("None", "AAC", "G1"), rd("None", "None", "None", xf="")]
    same = dict(uy=(8, 10), cy=(12, 16), gq=(2940, 98, 80))
    c["fragments"] = [
        rd("A", "AAA", "G1", pos=100, **same), rd("A", "AAA", "G1", pos=100, **same),
        rd("A", "AAA", "G1", pos=100, strand=1, **same), rd("A", "AAA", "G1", pos=200, **same),
        rd("A", "AAA", "G1", ref="chr2", pos=100, **same), un("A", "AAA", "G1", xf="CODING", nh=1, **same),
        rd("A", "AAC", "G1", pos=100, **same),
        rd("B", "AAA", "G1", pos=100), rd("B", "AAA", "G2", pos=100)]
    long_run = []
    for k in range(45):  # one triplet of 45 reads: longer than the runs the kernel resolves by scanning
        if k % 9 == 4:
            long_run.append(un("A", "AAA", "G1", xf="CODING", nh=1, **same))
        else:
            long_run.append(rd("A", "AAA", "G1", ref="chr%d" % (1 + k % 2), pos=100 + (k % 7) * 10, strand=(k // 7) % 2,
                               **same))
    long_run += [rd("A", "AAC", "G1", **same), rd("B", "AAA", "G1"), rd("B", "AAA", "G1")]
    c["long_run"] = long_run
    c["mitochondrial"] = [
        rd("C1", "AAA", "ENSG_MT1"), rd("C1", "AAC", "ENSG_MT1", pos=300), rd("C1", "AAG", "ENSG_MT1", pos=400),
        rd("C1", "AAA", "G3"), rd("C1", "AAC", "GX"), rd("C1", "AAT", "G2"),
        rd("C2", "AAA", "ENSG_MT1"), rd("C2", "AAC", "GX"), rd("C2", "AAG", "GX", pos=900),
        rd("C3", "AAA", "G3"), rd("C3", "AAC", "G2")]
    c["constant_streams"] = (
        [rd("A", u, "G1", uy=(7, 10), cy=(7, 10), gq=(3332, 100, 70)) for u in ("AAA", "AAC", "AAG", "AAT")] +
        [rd("B", u, "G1", uy=(1, 3), cy=(2, 3), gq=(100, 3, 1)) for u in ("AAA", "AAC", "AAG")] +
        [rd("C", u, "G2", uy=(10, 10), cy=(16, 16), gq=(98, 98, 0)) for u in ("AAA", "AAC")])
    c["zero_lengths"] = [
        rd("A", "AAA", "G1", cy=(0, 0)), rd("A", "AAC", "G1"), rd("A", "AAG", "G1", uy=(0, 0)),
        rd("B", "AAA", "G1", gq=(0, 0, 0)), rd("B", "AAC", "G1"),
        rd("C", "AAA", "G1"), rd("C", "AAC", "G1", cy=(0, 0), uy=(0, 0))]
    c["single_reads"] = [rd("A", "AAA", "G1"), rd("B", "AAA", "G1", xf="UTR"), un("C", "AAA", "G1"),
                         rd("D", "AAA", "G2", nh=2)]
    return c


def columns(reads):
    cols = {k: [r[k] for r in reads] for k in R.STR_FIELDS + R.INT_FIELDS}
    return R.stable_sorted(cols)


def shuffled_ties(cols, rng):
    n = len(cols["first"])
    order = sorted(range(n), key=lambda k: (cols["first"][k].encode(), cols["second"][k].encode(),
                                           cols["third"][k].encode(), rng.random()))
    return {k: [v[i] for i in order] for k, v in cols.items()}


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    src = sys.argv[1]
    tmp = tempfile.mkdtemp(prefix="tagsort_oracle_")
    drv = os.path.join(tmp, "driver.cpp")
    with open(drv, "w") as f:
        f.write(DRIVER)
    exe = os.path.join(tmp, "driver")
    subprocess.run(["g++", "-O1", "-std=c++17", "-I", src, "-o", exe, drv] +
                   [os.path.join(src, s) for s in ("metricgatherer.cpp", "mitochondrial_gene_selector.cpp",
                                                   "utilities.cpp")], check=True)
    gtf, names = os.path.join(HERE, "genes.gtf"), os.path.join(HERE, "mito_names.txt")
    with open(gtf, "w") as f:
        f.write(GTF)
    with open(names, "w") as f:
        f.write(NAMES)
    from sctools_amd import tagsort

    mito = tagsort.mitochondrial_gene_ids(gtf, names)
    rng = random.Random(5)
    for name, reads in cases().items():
        cols = columns(reads)
        lines = R.lines_of(cols)
        lp = os.path.join(HERE, name + ".lines.txt")
        with open(lp, "w") as f:
            f.write("".join(ln + "\n" for ln in lines))
        with open(os.path.join(HERE, name + ".json"), "w") as f:
            json.dump(cols, f, separators=(",", ":"))
            f.write("\n")
        for mt in ("cell", "gene"):
            out = os.path.join(HERE, "%s.%s.csv" % (name, mt))
            subprocess.run([exe, mt, lp, out] + ([gtf, names] if mt == "cell" else []), check=True,
                           stdout=subprocess.DEVNULL)
            want = open(out, newline="").read()
            got = R.gather(cols, mt, mito)
            assert got == want, "%s %s: the restatement differs from the reference\n%s\n%s" % (name, mt, got, want)
            for _ in range(25):
                assert R.gather(shuffled_ties(cols, rng), mt, mito) == want, "%s %s depends on tie order" % (name, mt)
        print("%-20s %3d reads" % (name, len(lines)))


if __name__ == "__main__":
    main()
