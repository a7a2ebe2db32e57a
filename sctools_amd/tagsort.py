"""
TagSort: the reference's native tag sort with cell or gene metrics (``fastqpreprocessing/src``:
``tagsort.cpp``, ``htslib_tagsort.cpp``, ``metricgatherer.{h,cpp}``,
``mitochondrial_gene_selector.cpp``), on the GPU.

Given the aligner's unsorted BAM, three tag names in a chosen order and a metric type, it writes
the metrics CSV the reference binary writes.  The per-read rule (``htslib_tagsort.cpp:106-218``) is
the decoder's ``tagsort`` mode; the order is ``sct_tag_sort`` over tag ids re-ranked in byte order
with ``None`` in its place; the gatherer (``metricgatherer.cpp:152-231``) is
``sct_tagsort_metrics`` (``csrc/tsmetrics.h``).  This module re-ranks the dictionaries, finishes
means, variances and ratios from the raw sums in plain double / float32 arithmetic (no contraction
can happen here) and prints them as the reference's streams do.

Equal triplets keep the BAM's order; the reference leaves their order undefined, so byte parity
holds for inputs whose result does not depend on it.
"""
import os
import re
from typing import Dict, List, Optional, Sequence, Set, Tuple

import numpy as np

from sctools_amd import _native as N

COMMON_HEADERS = (
    "n_reads", "noise_reads", "perfect_molecule_barcodes", "reads_mapped_exonic", "reads_mapped_intronic",
    "reads_mapped_utr", "reads_mapped_uniquely", "reads_mapped_multiple", "duplicate_reads", "spliced_reads",
    "antisense_reads", "molecule_barcode_fraction_bases_above_30_mean",
    "molecule_barcode_fraction_bases_above_30_variance", "genomic_reads_fraction_bases_quality_above_30_mean",
    "genomic_reads_fraction_bases_quality_above_30_variance", "genomic_read_quality_mean",
    "genomic_read_quality_variance", "n_molecules", "n_fragments", "reads_per_molecule", "reads_per_fragment",
    "fragments_per_molecule", "fragments_with_single_read_evidence", "molecules_with_single_read_evidence")
CELL_HEADERS = (
    "perfect_cell_barcodes", "reads_mapped_intergenic", "reads_unmapped", "reads_mapped_too_many_loci",
    "cell_barcode_fraction_bases_above_30_variance", "cell_barcode_fraction_bases_above_30_mean", "n_genes",
    "genes_detected_multiple_observations", "n_mitochondrial_genes", "n_mitochondrial_molecules",
    "pct_mitochondrial_molecules")
GENE_HEADERS = ("number_cells_detected_multiple", "number_cells_expressing")

ROLES = ("barcode", "umi", "gene")
MAX_THREADS = 30  # kMaxTagsortThreads (input_options.h:15)


class TagSortError(ValueError):
    """One of the reference's ``crash()`` conditions; the message is the reference's."""


# ---------------------------------------------------------------------------------------------
# mitochondrial gene ids (mitochondrial_gene_selector.cpp)
# ---------------------------------------------------------------------------------------------
def _split_fields(s: str, delim: str) -> List[str]:
    """splitStringToFields: std::getline per field, so no empty field after a trailing delimiter."""
    parts = s.split(delim)
    if parts and parts[-1] == "":
        parts.pop()
    return parts


def mitochondrial_gene_ids(gtf_file: str, mitochondrial_gene_names_filename: Optional[str] = None) -> Set[str]:
    """``gene_id`` of the GTF ``gene`` records whose ``gene_name`` is listed in the names file (blank and
    ``#`` lines skipped).  Without a names file: the names that start with ``mt-`` in any letter case,
    which the reference's help text promises (its binary stops instead: DESIGN.md §18).  The conditions the
    reference crashes on raise :class:`TagSortError`."""
    names = None
    if mitochondrial_gene_names_filename:
        try:
            with open(mitochondrial_gene_names_filename, "r", encoding="utf-8", errors="surrogateescape") as f:
                names = {ln for ln in f.read().split("\n") if ln and not ln.startswith("#")}
        except OSError:
            raise TagSortError("ERROR failed to open the mitochondrial gene names file named: %s"
                               % mitochondrial_gene_names_filename)
    try:
        f = open(gtf_file, "r", encoding="utf-8", errors="surrogateescape")
    except OSError:
        raise TagSortError("ERROR failed to open the GTF file named: %s" % gtf_file)
    ids: Set[str] = set()
    with f:
        for line in f.read().split("\n"):
            if not line or line.startswith("#"):
                continue
            fields = _split_fields(line, "\t")
            if len(fields) <= 8:
                raise TagSortError("Expected at least 9 tabbed fields, got %d" % len(fields))
            if fields[2] != "gene":
                continue
            gene_name = gene_id = ""
            for attrib in _split_fields(fields[8], ";"):
                key_and_val = _split_fields(attrib.lstrip(" \t\n\v\f\r"), " ")
                if len(key_and_val) != 2:
                    raise TagSortError("Expected 2 fields, found %d fields" % len(key_and_val))
                key, value = key_and_val[0], key_and_val[1].replace('"', "")
                if key == "gene_id":
                    gene_id = value
                if key == "gene_name":
                    gene_name = value
            if not gene_name:
                raise TagSortError("Malformed GTF file detected. Record is of type gene but does not "
                                   "have a gene_name in line:\n" + line)
            if (gene_name in names) if names is not None else (gene_name[:3].lower() == "mt-"):
                ids.add(gene_id)
    return ids


# ---------------------------------------------------------------------------------------------
# options (input_options.cpp:85-287, htslib_tagsort.cpp:417-453)
# ---------------------------------------------------------------------------------------------
def resolve_tag_order(barcode_tag: str, umi_tag: str, gene_tag: str, sequence: Sequence[Tuple[str, str]]):
    """The roles in sort position, from the tag options in the order they were given
    (``sequence``: (role, tag name) pairs).  ``tag_order`` is the reference's map from tag NAME to the
    map's size when the option was read; three distinct names are required, and a combination
    getTagOrder does not list falls back to barcode, umi, gene."""
    tag_order: Dict[str, int] = {}
    for _, name in sequence:
        tag_order[name] = len(tag_order)  # the size before the insertion, as the reference reads it
    if len(tag_order) != 3:
        raise TagSortError("ERROR:  Must have three distinct tags")
    if sorted(tag_order.values()) != [0, 1, 2]:
        raise TagSortError("Need tag indices 0 1 and 2")
    pos = (tag_order.get(barcode_tag, 0), tag_order.get(umi_tag, 0), tag_order.get(gene_tag, 0))
    listed = {(0, 2, 1): ("barcode", "gene", "umi"), (1, 0, 2): ("umi", "barcode", "gene"),
              (2, 0, 1): ("umi", "gene", "barcode"), (2, 1, 0): ("gene", "umi", "barcode"),
              (1, 2, 0): ("gene", "barcode", "umi")}
    return listed.get(pos, ROLES)


def check_options(bam_input, metric_type, gtf_file, metric_output=None, compute_metric=True,
                  temp_folder="/tmp/", alignments_per_thread=1000000, nthreads=1, tags=None, tag_sequence=None):
    """The reference's option checks, in its order, with its messages.  With ``tags`` (barcode, umi, gene
    tag names) and ``tag_sequence`` the three-distinct-tags check runs in its place and the roles in sort
    position are returned."""
    roles = None
    if not compute_metric:
        raise TagSortError("ERROR: The choice of either the sorted alignment info or metric computation "
                           "must be specified")
    if metric_output is not None and not metric_output:
        raise TagSortError("ERROR: Must specify --metric-output when specifying --compute-metric")
    if metric_type not in ("cell", "gene", "umi"):
        raise TagSortError('ERROR: --metric-type must be "cell", "gene", or "umi"')
    if metric_type == "cell" and not gtf_file:
        raise TagSortError('ERROR: The gtf file name must be provided with metric_type "cell"')
    if gtf_file and re.search(r".gz$", gtf_file, flags=re.I):
        raise TagSortError("ERROR: The gtf file must not be gzipped")
    if not bam_input:
        raise TagSortError("ERROR: Must specify a input file name")
    if not os.path.exists(bam_input):
        raise TagSortError("ERROR: bam_input %s is missing!" % bam_input)
    if not os.path.exists(temp_folder):
        raise TagSortError("ERROR: temp folder %s is missing!" % temp_folder)
    if tags is not None:
        roles = resolve_tag_order(tags[0], tags[1], tags[2], tag_sequence or [])
    if alignments_per_thread < 1000:
        raise TagSortError("ERROR: The number of alignments per thread must be at least 1000")
    if nthreads > MAX_THREADS or nthreads < 1:
        raise TagSortError("ERROR: The number of threads must be between 1 and %d" % MAX_THREADS)
    if metric_type == "umi":
        raise TagSortError("--metric-type umi is not supported: the reference's UmiMetricGatherer is empty")
    return roles


# ---------------------------------------------------------------------------------------------
# ranks: dictionary ids in byte order with "None" in its place; drop and mitochondrial flags
# ---------------------------------------------------------------------------------------------
def rank_dictionary(names: Sequence[Optional[str]]):
    """(new id per old id int32, the new dictionary's names): the names (``None`` = a missing tag, the
    string ``"None"``) ranked as std::string compares them, by unsigned byte."""
    as_bytes = [b"None" if s is None else s.encode("utf-8", "surrogateescape") for s in names]
    uniq = sorted(set(as_bytes))
    rank = {b: i for i, b in enumerate(uniq)}
    remap = np.fromiter((rank[b] for b in as_bytes), dtype=np.int32, count=len(as_bytes))
    return remap, [b.decode("utf-8", "surrogateescape") for b in uniq]


class Ranked:
    """The record columns with the three id columns in (first, second, third) position, and the per-id
    flags.  ``arrays`` are host columns (numpy) or the device decoder's tensors; the dictionaries are
    re-ranked on the host, over the names alone, and device id columns are renumbered where they lie."""

    def __init__(self, arrays: Dict[str, np.ndarray], names: Sequence[Sequence[Optional[str]]], roles: Sequence[str],
                 metric_type: str, mito_ids: Optional[Set[str]] = None):
        if sorted(roles) != sorted(ROLES):
            raise ValueError("tag_order must be a permutation of %r" % (ROLES,))
        by_role = {"barcode": ("cell", 0), "umi": ("umi", 1), "gene": ("gene", 2)}
        self.columns = dict(arrays)
        self.names: List[List[str]] = []
        for slot, role in zip(("cell", "umi", "gene"), roles):
            col, which = by_role[role]
            remap, ranked = rank_dictionary(list(names[which]) or [None])
            if hasattr(arrays[col], "is_cuda"):  # a device tensor: only the remap table travels
                import torch

                ids = arrays[col]
                self.columns[slot] = torch.index_select(torch.from_numpy(remap).to(ids.device), 0, ids)
            else:
                ids = np.asarray(arrays[col])
                self.columns[slot] = remap[ids].astype(np.int32) if ids.size else np.zeros(0, dtype=np.int32)
            self.names.append(ranked)
        first, third = self.names[0], self.names[2]
        self.first_drop = np.fromiter(((s == "None") or (metric_type == "gene" and "," in s) for s in first),
                                      dtype=np.uint8, count=len(first))
        mito = mito_ids or set()
        self.third_is_mito = np.fromiter((s in mito for s in third), dtype=np.uint8, count=len(third))


# ---------------------------------------------------------------------------------------------
# finishing and printing (metricgatherer.h:28-41, .cpp:7-12, 101-150, 278-325, 355-365)
# ---------------------------------------------------------------------------------------------
def _g10(x: float) -> str:
    """``ostream << setprecision(10) << x``.  Every NaN here comes from a 0 / 0 (a length of 0, or the
    mean of no reads), which the reference's x86 build prints with its sign."""
    x = float(x)
    if x != x:
        return "-nan"
    if x in (float("inf"), float("-inf")):
        return "inf" if x > 0 else "-inf"
    return "%.10g" % x


def _to_nan(x: float) -> str:
    """to_nan (metricgatherer.cpp:7-12): through float32; the -1 sentinel prints ``nan``."""
    with np.errstate(all="ignore"):
        x32 = np.float32(x)
    return "nan" if x32 == np.float32(-1) else _g10(float(x32))


def _mean(count: float, total: float) -> float:
    return total / count if count else float("nan")


def _variance(count: float, total: float, total2: float) -> float:
    if count < 2:
        return -1.0
    return total2 / (count - 1) - (total / count) * (total / (count - 1))


def _ratio(a: int, b: int) -> str:
    """``a / (float)b`` in float32, or the -1 of an empty histogram."""
    if b == 0:
        return "-1"
    with np.errstate(all="ignore"):
        return _g10(float(np.float32(a) / np.float32(b)))


def header(metric_type: str) -> str:
    extra = CELL_HEADERS if metric_type == "cell" else GENE_HEADERS
    return "".join("," + h for h in COMMON_HEADERS + extra) + "\n"


def format_rows(names: Sequence[str], ints: np.ndarray, sums: np.ndarray, metric_type: str) -> str:
    """The metrics CSV text (header and rows) of finished ``sct_tagsort_metrics`` rows."""
    out = [header(metric_type)]
    for r in range(len(names)):
        i = [int(v) for v in ints[r]]
        st = [[float(v) for v in sums[r][3 * s:3 * s + 3]] for s in range(4)]
        uy, gqf, gq, cy = st
        n_mol, n_frag, n_reads = i[N.TS_N_MOL], i[N.TS_N_FRAG], i[N.TS_N_READS]
        f = [names[r], str(n_reads), "0", str(i[N.TS_PERFECT_UMI]), str(i[N.TS_EXONIC]), str(i[N.TS_INTRONIC]),
             str(i[N.TS_UTR]), str(i[N.TS_UNIQUE]), str(i[N.TS_MULTIPLE]), str(i[N.TS_DUP]), str(i[N.TS_SPLICED]), "0",
             _g10(_mean(uy[0], uy[1])), _to_nan(_variance(*uy)),
             _g10(_mean(gqf[0], gqf[1])), _to_nan(_variance(*gqf)),
             _to_nan(_mean(gq[0], gq[1])), _to_nan(_variance(*gq)),
             str(n_mol), str(n_frag), _ratio(n_reads, n_mol), _ratio(n_reads, n_frag),
             _ratio(n_frag, n_mol), str(i[N.TS_FRAG_SINGLE]), str(i[N.TS_MOL_SINGLE])]
        if metric_type == "cell":
            mito_reads = i[N.TS_MITO_READS]
            # (n_mitochondrial_molecules / tot_molecules) * 100.0f with the reference's integer division
            pct = 100.0 if mito_reads > 0 and mito_reads // n_reads else 0.0
            f += [str(i[N.TS_PERFECT_CB]), str(i[N.TS_INTERGENIC]), str(i[N.TS_UNMAPPED]), "0",
                  _to_nan(_variance(*cy)), _g10(_mean(cy[0], cy[1])), str(i[N.TS_N_K1]), str(i[N.TS_K1_MULTI]),
                  str(i[N.TS_MITO_GENES]), str(mito_reads), _g10(pct)]
        else:
            f += [str(i[N.TS_K1_MULTI]), str(i[N.TS_N_K1])]
        out.append(",".join(f) + "\n")
    return "".join(out)


class Rows:
    """Finished rows: ``names`` (the final row's may be empty), ``ints`` [rows, 21] int64 and ``sums``
    [rows, 12] float64 as ``sct_tagsort_metrics`` returns them, on the host."""

    def __init__(self, names: List[str], ints: np.ndarray, sums: np.ndarray, metric_type: str):
        self.names, self.ints, self.sums, self.metric_type = names, ints, sums, metric_type

    def __len__(self) -> int:
        return len(self.names)

    def text(self) -> str:
        return format_rows(self.names, self.ints, self.sums, self.metric_type)


def write_metrics(rows: Rows, metric_output: str) -> str:
    """Writes the metrics CSV as the reference's streams print it; returns the path."""
    with open(metric_output, "w", encoding="utf-8", errors="surrogateescape", newline="") as f:
        f.write(rows.text())
    return metric_output


def gather(ranked: Ranked, metric_type: str, device=None, presorted: bool = False) -> Rows:
    """Sort (unless ``presorted``) and gather the ranked columns on the GPU; columns that are device
    tensors already are used as they are."""
    import torch

    from sctools_amd import engine as E

    eng = E.get_engine(device)
    with torch.cuda.device(eng.device):
        if all(torch.is_tensor(ranked.columns[c]) for c in N.RECORD_COLUMNS):
            cols = {c: ranked.columns[c].to(eng.device) for c in N.RECORD_COLUMNS}
        else:
            cols = E.to_device(ranked.columns, eng.device)
        dims = E.Dims(n_cell_ids=len(ranked.names[0]), n_gene_ids=len(ranked.names[2]), n_umi_ids=len(ranked.names[1]))
        if not presorted:
            cols = eng.tag_sort(cols, dims, "cell_umi_gene")
        drop = torch.from_numpy(ranked.first_drop).to(eng.device)
        mito = torch.from_numpy(ranked.third_is_mito).to(eng.device)
        ints, sums = eng.tagsort_metrics(cols, dims, metric_type, drop, mito)
        ints, sums = ints.cpu().numpy(), sums.cpu().numpy()
    first = ranked.names[0]
    names = [first[k] if k >= 0 else "" for k in ints[:, N.TS_NAME].tolist()]
    return Rows(names, ints, sums, metric_type)


class TagSort:
    """``TagSort(bam, metric_type, barcode_tag, umi_tag, gene_tag, ...).run(metric_output)``.

    ``tag_order`` gives the roles in sort position (the order of the tag options on the reference's
    command line).  ``decoder``: ``"auto"`` (the default) decodes the BAM on the GPU (libsct_gbam's
    TagSort mode) when that library and a GPU are there and the file is one it accepts, and with the host
    decoder otherwise (libsct_bam's ``tagsort`` mode, whose error is the reference-shaped one);
    ``"host"`` always uses the host decoder.  There is no device-only mode: ``"device"`` raises.  After
    ``decode()``, ``decoded_by`` is ``"device"`` or ``"host"``."""

    def __init__(self, bam_input: str, metric_type: str, barcode_tag: str, umi_tag: str, gene_tag: str,
                 tag_order: Sequence[str] = ROLES, gtf_file: Optional[str] = None,
                 mitochondrial_gene_names_filename: Optional[str] = None, device=None, decoder: str = "auto"):
        check_options(bam_input, metric_type, gtf_file)
        if len({barcode_tag, umi_tag, gene_tag}) != 3:
            raise TagSortError("ERROR:  Must have three distinct tags")
        if sorted(tag_order) != sorted(ROLES):
            raise ValueError("tag_order must be a permutation of %r" % (ROLES,))
        if decoder not in ("auto", "host", "device"):
            raise ValueError("decoder must be 'auto', 'host' or 'device'")
        if decoder == "device":
            raise NotImplementedError("there is no device-only mode: decoder='auto' decodes on the device and "
                                      "falls back to the host decoder for a file the device declines")
        self.bam_input, self.metric_type = bam_input, metric_type
        self.tags = (barcode_tag, umi_tag, gene_tag)
        self.tag_order = tuple(tag_order)
        self.gtf_file, self.names_file = gtf_file, mitochondrial_gene_names_filename
        self.device = device
        self.decoder = decoder
        self.decoded_by: Optional[str] = None

    def _device_columns(self, timings: Optional[dict]):
        """The columns decoded by libsct_gbam.so, or None (no library, no GPU, tag names it cannot take, or a
        file it declines: typed tag values, non-ASCII strings, records past the columns' width ...)."""
        import torch

        from sctools_amd import gbam

        if not gbam.available() or not torch.cuda.is_available():
            return None
        if any(len(t) != 2 or not t.isascii() or "\0" in t for t in self.tags):
            return None
        return gbam.decode(self.bam_input, "tagsort", device=self.device, timings=timings, tags=self.tags)

    def decode(self, timings: Optional[dict] = None) -> Ranked:
        """``timings``: filled with the device decoder's stages (``gbam.STAGES``) when it decodes the file."""
        from sctools_amd import bamnative

        mito = mitochondrial_gene_ids(self.gtf_file, self.names_file) if self.metric_type == "cell" else None
        got = self._device_columns(timings) if self.decoder == "auto" else None
        self.decoded_by = "host" if got is None else "device"
        arrays, names = got if got is not None else bamnative.decode(self.bam_input, "tagsort", tags=self.tags)
        return Ranked(arrays, names, self.tag_order, self.metric_type, mito)

    def run(self, metric_output: str, timings: Optional[dict] = None):
        rows = gather(self.decode(timings), self.metric_type, device=self.device)
        return rows, write_metrics(rows, metric_output)


def main(argv=None) -> int:
    """``python -m sctools_amd TagSort``: the reference's option names (input_options.cpp:85-130)."""
    import argparse

    class _Tag(argparse.Action):
        def __call__(self, parser, namespace, value, option_string=None):
            setattr(namespace, self.dest, value)
            namespace.tag_sequence = getattr(namespace, "tag_sequence", None) or []
            namespace.tag_sequence.append((self.dest.split("_")[0], value))

    p = argparse.ArgumentParser(prog="TagSort", description="Sort the alignments of a BAM by three tags and write "
                                "the cell or gene metrics of the sorted reads (the reference's native TagSort)")
    p.add_argument("--compute-metric", action="store_true", help="compute the metrics")
    p.add_argument("--output-sorted-info", action="store_true", help="not supported (DESIGN.md §7)")
    p.add_argument("--bam-input", default="", help="input BAM")
    p.add_argument("--gtf-file", default="", help="GTF (not gzipped); required for --metric-type cell")
    p.add_argument("--temp-folder", default="/tmp/", help="checked to exist, otherwise unused")
    p.add_argument("--sorted-output", default="", help="not supported (DESIGN.md §7)")
    p.add_argument("--metric-output", default="", help="metrics CSV to write")
    p.add_argument("--alignments-per-thread", type=int, default=1000000, help="checked (>= 1000), otherwise unused")
    p.add_argument("--nthreads", type=int, default=1, help="checked (1..%d), otherwise unused" % MAX_THREADS)
    p.add_argument("--barcode-tag", action=_Tag, default="", help="cell barcode tag")
    p.add_argument("--umi-tag", action=_Tag, default="", help="UMI tag")
    p.add_argument("--gene-tag", action=_Tag, default="", help="gene tag; the order of the three tag options "
                   "is the sort order")
    p.add_argument("--metric-type", default="", help='"cell" or "gene"')
    p.add_argument("--mitochondrial-gene-names-filename", default="", help="gene names to count as mitochondrial, "
                   "one per line (default: names starting with mt-)")
    p.add_argument("--device", default=None, help="GPU index or torch device (default: current GPU)")
    p.add_argument("--decoder", default="auto", choices=["auto", "host"], help="auto: the BAM is decoded on the "
                   "GPU, or by the host decoder when the device path declines it; host: always the host decoder")
    a = p.parse_args(argv)
    if a.output_sorted_info:
        raise TagSortError("--output-sorted-info is not supported: the record does not carry the CY quality sum of "
                           "its seventh field, and the reference leaves the order of equal triplets undefined")
    roles = check_options(a.bam_input, a.metric_type, a.gtf_file, metric_output=a.metric_output,
                          compute_metric=a.compute_metric, temp_folder=a.temp_folder,
                          alignments_per_thread=a.alignments_per_thread, nthreads=a.nthreads,
                          tags=(a.barcode_tag, a.umi_tag, a.gene_tag),
                          tag_sequence=getattr(a, "tag_sequence", None))
    TagSort(a.bam_input, a.metric_type, a.barcode_tag, a.umi_tag, a.gene_tag, tag_order=roles,
            gtf_file=a.gtf_file or None, mitochondrial_gene_names_filename=a.mitochondrial_gene_names_filename or None,
            device=a.device, decoder=a.decoder).run(a.metric_output)
    return 0
