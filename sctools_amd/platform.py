"""
Command-line entry points for the metric path -- same names, flags and return
codes as the reference's ``GenericPlatform`` metric commands
(``/root/reference/src/sctools/platform.py:225-381``; console scripts
``setup.py:42-49``):

  CalculateCellMetrics -i BAM -o STEM [-a GTF]
  CalculateGeneMetrics -i BAM -o STEM
  MergeCellMetrics FILES... -o STEM
  MergeGeneMetrics FILES... -o STEM
  SplitBam -b BAM... -p PREFIX -t TAG... [-s MB] [--num-processes N] [--drop-missing]  (platform.py:153-223)
  TagSortBam -i BAM -o BAM [-t TAG...]...                               (platform.py:60-97)
  VerifyBamSort -i BAM [-t TAG...]...                                   (platform.py:100-143)
  CreateCountMatrix -b BAM -o PREFIX -a GTF [-c TAG -m TAG -g TAG -n]   (platform.py:384-470)
  MergeCountMatrices -i PREFIX... -o STEM                              (platform.py:475-516)

  Attach10xBarcodes --r1 FASTQ --u2 BAM -o BAM [--i1 FASTQ] [-w WHITELIST]                 (platform.py:579-758)
  AttachBarcodes --r1 FASTQ --u2 BAM -o BAM [--i1 FASTQ] [-w WHITELIST]
                 [--{sample,cell,molecule}-barcode-start-position N --{...}-barcode-length N]  (platform.py:761-1126)

An addition: ``CorrectBarcodes -i BAM -o BAM --whitelist FILE [--device N]`` sets every record's
``CB`` from its ``CR`` and the whitelist (``ErrorsToCorrectBarcodesMap.correct_bam``,
barcode.py:357-379), for a BAM that already carries ``CR``.

From the reference's fastqpreprocessing tools: ``FastqMetrics --R1 FASTQ [--R1 FASTQ ...] --read-structure S
--sample-id PREFIX [--white-list FILE] [--device N]`` (``fastq_metrics.cpp``; ``sctools_amd/fastq_metrics.py``).

``FastqProcess --R1 FASTQ --R2 FASTQ [--I1 FASTQ] (each repeatable) [--white-list FILE] --barcode-length N
--umi-length N | --read-structure S [--sample-id ID] [--output-format BAM|FASTQ] [--bam-size GIB]
[--num-shards N] [--output-dir DIR] [--device N]`` (``fastqprocess.cpp``, ``fastq_slideseq.cpp``;
``sctools_amd/fastq_process.py``); ``FastqSlideseq`` is the same command.

The four FASTQ commands (``Attach10xBarcodes``, ``AttachBarcodes``, ``FastqMetrics``, ``FastqProcess`` /
``FastqSlideseq``) take ``--inflate auto|host``: with ``auto`` (the default) a BGZF-compressed FASTQ is inflated
on the GPU, with ``host`` by Python's gzip like every other file (``fastq.TextWindows``).

``TagSort --bam-input BAM --metric-type cell|gene --compute-metric --metric-output CSV --barcode-tag T
--umi-tag T --gene-tag T (their order is the sort order) [--gtf-file GTF] [--mitochondrial-gene-names-filename FILE]
[--temp-folder DIR] [--alignments-per-thread N] [--nthreads N] [--device N] [--decoder auto|host]`` (``tagsort.cpp``,
``metricgatherer.cpp``; ``sctools_amd/tagsort.py``).

New flags are optional only: ``--float-mode {welford,exact}``, ``--device``, ``--devices N``
(spread the entity runs over GPUs 0..N-1, one host thread each; same output) and, on
CalculateCellMetrics, ``--gene-output-filestem STEM`` (also write the gene rows of the same
cell-sorted file, as TagSortBam by gene + CalculateGeneMetrics would give them; with
``--devices N`` the per-device gene partials are summed by an RCCL all-reduce -- the
SplitBam / MergeGeneMetrics workflow in one command).
Run as ``python -m sctools_amd <Command> [args]``.
"""

import argparse
from typing import Iterable, Set

from sctools_amd import bam, consts, count, fastq, gtf, metrics


def _engine_args(parser):
    parser.add_argument("--float-mode", default="welford", choices=["welford", "exact"],
                        help="welford: bit-identical to sctools (default); exact: order-free exact sums")
    parser.add_argument("--device", default=None, help="torch device (default: current GPU)")
    parser.add_argument("--devices", type=int, default=None,
                        help="spread the work over GPUs 0..N-1 (one host thread each); output unchanged")


class GenericPlatform:
    @classmethod
    def calculate_gene_metrics(cls, args: Iterable[str] = None) -> int:
        parser = argparse.ArgumentParser()
        parser.add_argument("-i", "--input-bam", required=True, help="Input bam file name.")
        parser.add_argument("-o", "--output-filestem", required=True, help="Output file stem.")
        _engine_args(parser)
        args = parser.parse_args(args) if args is not None else parser.parse_args()
        g = metrics.gatherer.GatherGeneMetrics(args.input_bam, args.output_filestem,
                                               float_mode=args.float_mode, device=args.device,
                                               devices=args.devices)
        g.extract_metrics()
        return 0

    @classmethod
    def calculate_cell_metrics(cls, args: Iterable[str] = None) -> int:
        parser = argparse.ArgumentParser()
        parser.add_argument("-i", "--input-bam", required=True, help="Input bam file name.")
        parser.add_argument("-o", "--output-filestem", required=True, help="Output file stem.")
        parser.add_argument("-a", "--gtf-annotation-file", required=False, default=None,
                            help="gtf annotation file that bam_file was aligned against")
        parser.add_argument("--gene-output-filestem", default=None,
                            help="also write the gene metrics of this cell-sorted file (grouped by gene, "
                                 "exact-sum floats) from the same pass")
        _engine_args(parser)
        args = parser.parse_args(args) if args is not None else parser.parse_args()
        mito: Set[str] = set()
        if args.gtf_annotation_file:
            mito = gtf.get_mitochondrial_gene_names(args.gtf_annotation_file)
        if args.gene_output_filestem:
            g = metrics.gatherer.GatherCellAndGeneMetrics(args.input_bam, args.output_filestem,
                                                          args.gene_output_filestem, mito,
                                                          float_mode=args.float_mode, devices=args.devices or 1)
        else:
            g = metrics.gatherer.GatherCellMetrics(args.input_bam, args.output_filestem, mito,
                                                   float_mode=args.float_mode, device=args.device,
                                                   devices=args.devices)
        g.extract_metrics()
        return 0

    @classmethod
    def merge_gene_metrics(cls, args: Iterable[str] = None) -> int:
        parser = argparse.ArgumentParser()
        parser.add_argument("metric_files", nargs="+", help="Input metric files")
        parser.add_argument("-o", "--output-filestem", required=True, help="Output file stem.")
        args = parser.parse_args(args) if args is not None else parser.parse_args()
        metrics.merge.MergeGeneMetrics(args.metric_files, args.output_filestem).execute()
        return 0

    @classmethod
    def merge_cell_metrics(cls, args: Iterable[str] = None) -> int:
        parser = argparse.ArgumentParser()
        parser.add_argument("metric_files", nargs="+", help="Input metric files")
        parser.add_argument("-o", "--output-filestem", required=True, help="Output file stem.")
        args = parser.parse_args(args) if args is not None else parser.parse_args()
        metrics.merge.MergeCellMetrics(args.metric_files, args.output_filestem).execute()
        return 0


    @classmethod
    def split_bam(cls, args: Iterable[str] = None) -> int:
        """SplitBam (platform.py:153-223): prints the chunk file names, space-separated."""
        parser = argparse.ArgumentParser()
        parser.add_argument("-b", "--bamfile", nargs="+", required=True, help="input bamfile")
        parser.add_argument("-p", "--output-prefix", required=True, help="prefix for output chunks")
        parser.add_argument("-s", "--subfile-size", required=False, default=1000, type=float,
                            help="approximate size target for each subfile (in MB)")
        parser.add_argument("--num-processes", required=False, default=None, type=int,
                            help="Number of processes to parallelize over")
        parser.add_argument("-t", "--tags", nargs="+",
                            help="tag(s) to split bamfile over. Tags are checked sequentially, and tags after the "
                                 "first are only checked if the first tag is not present.")
        parser.set_defaults(raise_missing=True)
        parser.add_argument("--drop-missing", action="store_false",
                            help="drop records without tag specified by -t/--tag (default behavior is to raise an "
                                 "exception")
        args = parser.parse_args(args) if args is not None else parser.parse_args()
        filenames = bam.split(args.bamfile, args.output_prefix, args.tags, approx_mb_per_split=args.subfile_size,
                              raise_missing=args.drop_missing, num_processes=args.num_processes)
        print(" ".join(filenames))
        return 0

    @classmethod
    def tag_sort_bam(cls, args: Iterable[str] = None) -> int:
        """TagSortBam (platform.py:60-97): the BAM sorted by the tags (zero or more), then the query
        name; the order is computed on the GPU, the records are rewritten natively."""
        parser = argparse.ArgumentParser(description="Sorts bam by list of zero or more tags, followed by query name")
        parser.add_argument("-i", "--input_bam", required=True, help="input bamfile")
        parser.add_argument("-o", "--output_bam", required=True, help="output bamfile")
        parser.add_argument("-t", "--tags", nargs="+", action="append",
                            help="tag(s) to sort by, separated by space, e.g. -t CB GE UB")
        parser.add_argument("--device", default=None, help="torch device (default: current GPU)")
        args = parser.parse_args(args) if args is not None else parser.parse_args()
        bam.tag_sort_bam(args.input_bam, args.output_bam, cls.get_tags(args.tags), device=args.device)
        return 0

    @classmethod
    def verify_bam_sort(cls, args: Iterable[str] = None) -> int:
        """VerifyBamSort (platform.py:100-143): raises bam.SortError unless the BAM is sorted by
        the tags (zero or more), then the query name; the check runs on the GPU."""
        parser = argparse.ArgumentParser(
            description="Verifies whether bam is sorted by the list of zero or more tags, followed by query name")
        parser.add_argument("-i", "--input_bam", required=True, help="input bamfile")
        parser.add_argument("-t", "--tags", nargs="+", action="append",
                            help="tag(s) to use to verify sorting, separated by space, e.g. -t CB GE UB")
        parser.add_argument("--device", default=None, help="torch device (default: current GPU)")
        args = parser.parse_args(args) if args is not None else parser.parse_args()
        tags = cls.get_tags(args.tags)
        bam.verify_bam_sort(args.input_bam, tags, device=args.device)
        print("{0} is correctly sorted by {1} and query name".format(args.input_bam, tags))
        return 0

    @classmethod
    def get_tags(cls, raw_tags) -> list:
        """-t A B -t C -> [A, B, C] (platform.py:145-150)."""
        return [t for group in (raw_tags or []) for t in group]

    @classmethod
    def bam_to_count_matrix(cls, args: Iterable[str] = None) -> int:
        """CreateCountMatrix (platform.py:384-470): query-name-grouped tagged BAM -> CSR count matrix."""
        parser = argparse.ArgumentParser()
        parser.set_defaults(cell_barcode_tag=consts.CELL_BARCODE_TAG_KEY,
                            molecule_barcode_tag=consts.MOLECULE_BARCODE_TAG_KEY,
                            gene_name_tag=consts.GENE_NAME_TAG_KEY, sn_rna_seq_mode=False)
        parser.add_argument("-b", "--bam-file", help="input_bam_file", required=True)
        parser.add_argument("-o", "--output-prefix", help="file stem for count matrix", required=True)
        parser.add_argument("-a", "--gtf-annotation-file", required=True,
                            help="gtf annotation file that bam_file was aligned against")
        parser.add_argument("-c", "--cell-barcode-tag",
                            help="tag that identifies the cell barcode (default = %s)" % consts.CELL_BARCODE_TAG_KEY)
        parser.add_argument("-m", "--molecule-barcode-tag", help="tag that identifies the molecule barcode "
                            "(default = %s)" % consts.MOLECULE_BARCODE_TAG_KEY)
        parser.add_argument("-g", "--gene-id-tag",
                            help="tag that identifies the gene name (default = %s)" % consts.GENE_NAME_TAG_KEY)
        parser.add_argument("-n", "--sn-rna-seq-mode", action="store_true", help="snRNA Seq mode (default = False)")
        parser.add_argument("--device", default=None, help="torch device (default: current GPU)")
        args = parser.parse_args(args) if args is not None else parser.parse_args()
        open_mode = "r" if args.bam_file.endswith(".sam") else "rb"
        gene_name_to_index = gtf.extract_gene_names(args.gtf_annotation_file)
        gene_locations = gtf.extract_extended_gene_names(args.gtf_annotation_file) if args.sn_rna_seq_mode else None
        matrix = count.CountMatrix.from_sorted_tagged_bam(
            bam_file=args.bam_file, gene_name_to_index=gene_name_to_index,
            chromosomes_gene_locations_extended=gene_locations, cell_barcode_tag=args.cell_barcode_tag,
            molecule_barcode_tag=args.molecule_barcode_tag, gene_name_tag=args.gene_id_tag, open_mode=open_mode,
            device=args.device)
        matrix.save(args.output_prefix)
        return 0

    @classmethod
    def merge_count_matrices(cls, args: Iterable[str] = None) -> int:
        """MergeCountMatrices (platform.py:475-516)."""
        parser = argparse.ArgumentParser()
        parser.add_argument("-i", "--input-prefixes", nargs="+", help="prefix for count matrices to be concatenated. "
                            "e.g. test_counts for test_counts.npz, test_counts_col_index.npy, and "
                            "test_counts_row_index.npy")
        parser.add_argument("-o", "--output-stem", help="file stem for merged csr matrix", required=True)
        args = parser.parse_args(args) if args is not None else parser.parse_args()
        count.CountMatrix.merge_matrices(args.input_prefixes).save(args.output_stem)
        return 0

    @classmethod
    def correct_barcodes(cls, args: Iterable[str] = None) -> int:
        """CorrectBarcodes (an addition): CB from CR and a whitelist, the lookups on the GPU."""
        from sctools_amd import barcode

        parser = argparse.ArgumentParser(description="Sets CB to the whitelist barcode within Hamming distance 1 "
                                                     "of CR, or to CR itself where there is none")
        parser.add_argument("-i", "--input-bam", required=True, help="input bamfile with CR tags")
        parser.add_argument("-o", "--output-bam", required=True, help="output bamfile")
        parser.add_argument("--whitelist", required=True, help="text file, one barcode per line")
        parser.add_argument("--device", default=None, help="GPU index or torch device (default: current GPU)")
        args = parser.parse_args(args) if args is not None else parser.parse_args()
        corrector = barcode.ErrorsToCorrectBarcodesMap.single_hamming_errors_from_whitelist(args.whitelist,
                                                                                            device=args.device)
        corrector.correct_bam(args.input_bam, args.output_bam)
        return 0

    @classmethod
    def fastq_metrics(cls, args: Iterable[str] = None) -> int:
        """FastqMetrics (the reference's fastqpreprocessing ``fastq_metrics`` tool): reads per cell barcode
        and per UMI and their position weight matrices, counted on the GPU; four text files."""
        from sctools_amd import fastq_metrics

        parser = argparse.ArgumentParser(description="Reads per distinct cell barcode and UMI of R1 FASTQ files, and the "
                                                     "base counts per barcode position")
        parser.add_argument("--R1", action="append", required=True, help="R1 FASTQ file (plain or compressed); may be "
                            "given several times, the files are counted together")
        parser.add_argument("--read-structure", required=True, help="e.g. 16C10M or 8C18X6C9M1X: C cell barcode, "
                            "M UMI, any other letter skipped")
        parser.add_argument("--sample-id", required=True, help="prefix of the four output files")
        parser.add_argument("--white-list", default=None, help="accepted and unused, as in the reference")
        parser.add_argument("--device", default=None, help="GPU index or torch device (default: current GPU)")
        parser.add_argument("--inflate", default=fastq.DEFAULT_INFLATE, choices=list(fastq.INFLATE_MODES),
                            help="who inflates BGZF-compressed FASTQ: auto = the GPU (any other file is read on the "
                                 "host), host = the host for every file")
        args = parser.parse_args(args) if args is not None else parser.parse_args()
        result = fastq_metrics.FastqMetrics(args.R1, args.read_structure, whitelist=args.white_list,
                                            inflate=args.inflate).compute(device=args.device)
        result.write(args.sample_id)
        return 0

    @classmethod
    def fastq_process(cls, args: Iterable[str] = None) -> int:
        """FastqProcess / FastqSlideseq (the reference's fastqpreprocessing ``fastqprocess`` and
        ``fastq_slideseq`` tools): FASTQ triples to unaligned BAM or FASTQ shards, one cell in one shard."""
        from sctools_amd import fastq_process

        parser = argparse.ArgumentParser(description="Cut the cell barcode and the UMI out of R1, correct the cell "
                                                     "barcode, and write every read of R2 to the shard its barcode picks")
        parser.add_argument("--R1", action="append", required=True, help="barcode read FASTQ (plain or compressed); "
                            "repeatable, file k goes with --R2 k and --I1 k")
        parser.add_argument("--R2", action="append", required=True, help="cDNA read FASTQ; repeatable")
        parser.add_argument("--I1", action="append", default=None, help="index read FASTQ; repeatable, optional")
        parser.add_argument("--white-list", default=None, help="cell barcode whitelist, one barcode per line")
        parser.add_argument("--barcode-length", type=int, default=None, help="cell barcode bases at the start of R1")
        parser.add_argument("--umi-length", type=int, default=None, help="UMI bases behind the cell barcode")
        parser.add_argument("--read-structure", default=None, help="instead of the two lengths, e.g. 8C18X6C9M1X: "
                            "C cell barcode, M UMI, any other letter skipped")
        parser.add_argument("--sample-id", default="", help="SM of the BAM read group")
        parser.add_argument("--output-format", default="BAM", choices=["BAM", "FASTQ"])
        parser.add_argument("--bam-size", type=float, default=1.0, help="GiB of input per shard (default 1.0)")
        parser.add_argument("--num-shards", type=int, default=None, help="number of shards (default: from --bam-size)")
        parser.add_argument("--output-dir", default=".", help="where the shards go (default: the current directory)")
        parser.add_argument("--device", default=None, help="GPU index or torch device (default: current GPU)")
        parser.add_argument("--inflate", default=fastq.DEFAULT_INFLATE, choices=list(fastq.INFLATE_MODES),
                            help="who inflates BGZF-compressed FASTQ: auto = the GPU (any other file is read on the "
                                 "host), host = the host for every file")
        args = parser.parse_args(args) if args is not None else parser.parse_args()
        result = fastq_process.FastqProcess(
            args.R1, args.R2, i1_files=args.I1, whitelist=args.white_list, barcode_length=args.barcode_length,
            umi_length=args.umi_length, read_structure=args.read_structure, sample_id=args.sample_id,
            output_format=args.output_format, bam_size=args.bam_size, num_shards=args.num_shards,
            output_dir=args.output_dir, inflate=args.inflate).run(device=args.device)
        print("Total barcodes:%d\n correct:%d\ncorrected:%d\nuncorrectible:%d\nuncorrected:%f"
              % (result.n_reads, result.n_correct, result.n_corrected, result.n_uncorrectable,
                 100.0 * result.n_uncorrectable / max(result.n_reads, 1)))
        return 0

    @classmethod
    def tag_sort(cls, args: Iterable[str] = None) -> int:
        """TagSort (the reference's fastqpreprocessing ``TagSort`` binary): the unsorted BAM ordered by three
        tags and the cell or gene metrics of the sorted reads, gathered on the GPU; one CSV."""
        from sctools_amd import tagsort

        return tagsort.main(args)


class TenXV2(GenericPlatform):
    """10x Genomics v2: the metric commands (platform.py:579) and ``Attach10xBarcodes``.

    The three barcodes of a 10x v2 read pair: cell and molecule barcode in read 1, the sample barcode in
    the i7 index read, with the tags they are attached under.
    """

    cell_barcode = fastq.EmbeddedBarcode(start=0, end=16, quality_tag=consts.QUALITY_CELL_BARCODE_TAG_KEY,
                                         sequence_tag=consts.RAW_CELL_BARCODE_TAG_KEY)
    molecule_barcode = fastq.EmbeddedBarcode(start=16, end=26, quality_tag=consts.QUALITY_MOLECULE_BARCODE_TAG_KEY,
                                             sequence_tag=consts.RAW_MOLECULE_BARCODE_TAG_KEY)
    sample_barcode = fastq.EmbeddedBarcode(start=0, end=8, quality_tag=consts.QUALITY_SAMPLE_BARCODE_TAG_KEY,
                                           sequence_tag=consts.RAW_SAMPLE_BARCODE_TAG_KEY)

    @classmethod
    def _tag_bamfile(cls, input_bamfile_name: str, output_bamfile_name: str, tag_generators, device=None,
                     inflate: str = fastq.DEFAULT_INFLATE) -> None:
        bam.Tagger(input_bamfile_name, device=device, inflate=inflate).tag(output_bamfile_name, tag_generators)

    @classmethod
    def _make_tag_generators(cls, r1, i1=None, whitelist=None) -> list:
        """Cell and molecule barcodes from ``r1`` (with ``CB`` when there is a whitelist), then the sample
        barcode from ``i1`` (platform.py:653-704)."""
        if whitelist is not None:
            generators = [fastq.BarcodeGeneratorWithCorrectedCellBarcodes(
                fastq_files=r1, embedded_cell_barcode=cls.cell_barcode, whitelist=whitelist,
                other_embedded_barcodes=[cls.molecule_barcode])]
        else:
            generators = [fastq.EmbeddedBarcodeGenerator(
                fastq_files=r1, embedded_barcodes=[cls.cell_barcode, cls.molecule_barcode])]
        if i1 is not None:
            generators.append(fastq.EmbeddedBarcodeGenerator(fastq_files=i1, embedded_barcodes=[cls.sample_barcode]))
        return generators

    @classmethod
    def attach_barcodes(cls, args: Iterable[str] = None) -> int:
        """Attach10xBarcodes (platform.py:706-758): the barcodes of the read 1 (and i7) FASTQ attached to
        the records of the unaligned read 2 BAM; extraction and correction on the GPU."""
        parser = argparse.ArgumentParser()
        parser.add_argument("--r1", required=True, help="FASTQ of read 1 (10x v2): cell barcode in bases 0-15, molecule barcode in bases 16-25")
        parser.add_argument("--u2", required=True, help="unaligned BAM of read 2 (the cDNA), one record per FASTQ record "
                            "in the same order, e.g. from picard FastqToSam")
        parser.add_argument("--i1", default=None, help="FASTQ of the i7 index read; when given, the sample barcode (bases 0-7) is attached too")
        parser.add_argument("-o", "--output-bamfile", required=True, help="the tagged BAM to write")
        parser.add_argument("-w", "--whitelist", default=None,
                            help="cell barcode whitelist, one barcode per line; with it, CB is set where the raw cell "
                                 "barcode is on the list or one substitution away from it")
        parser.add_argument("--device", default=None, help="GPU index or torch device (default: current GPU)")
        parser.add_argument("--inflate", default=fastq.DEFAULT_INFLATE, choices=list(fastq.INFLATE_MODES),
                            help="who inflates BGZF-compressed FASTQ: auto = the GPU (any other file is read on the "
                                 "host), host = the host for every file")
        args = parser.parse_args(args) if args is not None else parser.parse_args()
        cls._tag_bamfile(args.u2, args.output_bamfile, cls._make_tag_generators(args.r1, args.i1, args.whitelist),
                         device=args.device, inflate=args.inflate)
        return 0


class BarcodePlatform(GenericPlatform):
    """``AttachBarcodes`` (platform.py:761-1126): ``Attach10xBarcodes`` with the position and length of
    the sample, cell and molecule barcode given on the command line."""

    cell_barcode = None
    molecule_barcode = None
    sample_barcode = None

    @classmethod
    def _validate_barcode_args(cls, args):
        """Every barcode has both a start position and a length or neither, a sample barcode has an i7
        file to come from, and the molecule barcode starts at or after the cell barcode's end."""
        cls._validate_barcode_length_and_position(args.cell_barcode_start_pos, args.cell_barcode_length)
        cls._validate_barcode_length_and_position(args.molecule_barcode_start_pos, args.molecule_barcode_length)
        cls._validate_barcode_length_and_position(args.sample_barcode_start_pos, args.sample_barcode_length)
        if args.i1 is None and args.sample_barcode_length:
            raise argparse.ArgumentError(None, "An i7 index fastq file must be given to attach a sample barcode")
        if args.cell_barcode_length and args.molecule_barcode_length:
            cls._validate_barcode_input(args.molecule_barcode_start_pos,
                                        args.cell_barcode_start_pos + args.cell_barcode_length)
        return args

    @classmethod
    def _validate_barcode_length_and_position(cls, barcode_start_position, barcode_length):
        has_position = bool(barcode_start_position) or barcode_start_position == 0
        if has_position != bool(barcode_length):
            raise argparse.ArgumentError(
                None, "Invalid position/length, both position and length must be provided by the user together")

    @classmethod
    def _validate_barcode_input(cls, given_value, min_value):
        if given_value < min_value:
            raise argparse.ArgumentTypeError("Invalid barcode length/position")
        return given_value

    @classmethod
    def _validate_barcode_start_pos(cls, given_value):
        return cls._validate_barcode_input(int(given_value), 0)

    @classmethod
    def _validate_barcode_length(cls, given_value):
        return cls._validate_barcode_input(int(given_value), 1)

    @classmethod
    def _tag_bamfile(cls, input_bamfile_name: str, output_bamfile_name: str, tag_generators, device=None,
                     inflate: str = fastq.DEFAULT_INFLATE) -> None:
        bam.Tagger(input_bamfile_name, device=device, inflate=inflate).tag(output_bamfile_name, tag_generators)

    @classmethod
    def _make_tag_generators(cls, r1, i1=None, whitelist=None) -> list:
        """The generators in the reference's order (platform.py:974-1001), the sample barcode's first.  As
        there, every generator reads ``r1``: with ``i1`` given, the sample barcode is cut from read 1
        (DESIGN.md section 14)."""
        generators = []
        if i1:
            generators.append(fastq.EmbeddedBarcodeGenerator(fastq_files=r1, embedded_barcodes=[cls.sample_barcode]))
        if whitelist:
            kwargs = {"fastq_files": r1, "whitelist": whitelist}
            if cls.cell_barcode:
                kwargs["embedded_cell_barcode"] = cls.cell_barcode
            if cls.molecule_barcode:
                kwargs["other_embedded_barcodes"] = [cls.molecule_barcode]
            generators.append(fastq.BarcodeGeneratorWithCorrectedCellBarcodes(**kwargs))
        else:
            generators.append(fastq.EmbeddedBarcodeGenerator(
                fastq_files=r1, embedded_barcodes=[b for b in (cls.cell_barcode, cls.molecule_barcode) if b]))
        return generators

    @classmethod
    def attach_barcodes(cls, args: Iterable[str] = None) -> int:
        parser = argparse.ArgumentParser()
        parser.add_argument("--r1", required=True, help="FASTQ of read 1, which holds the cell and the molecule barcode")
        parser.add_argument("--u2", required=True, help="unaligned BAM of read 2, one record per FASTQ record in the same "
                            "order, e.g. from picard FastqToSam")
        parser.add_argument("-o", "--output-bamfile", required=True, help="the tagged BAM to write")
        parser.add_argument("-w", "--whitelist", default=None,
                            help="cell barcode whitelist, one barcode per line; with it, CB is set where the raw cell "
                                 "barcode is on the list or one substitution away from it")
        parser.add_argument("--i1", default=None, help="FASTQ of the i7 index read; required with a sample barcode")
        for name, where in (("sample", "sample"), ("cell", "cell"), ("molecule", "molecule")):
            parser.add_argument("--%s-barcode-start-position" % name, dest="%s_barcode_start_pos" % name, default=None,
                                type=cls._validate_barcode_start_pos,
                                help="0-based position of the first base of the %s barcode" % where)
            parser.add_argument("--%s-barcode-length" % name, dest="%s_barcode_length" % name, default=None,
                                type=cls._validate_barcode_length,
                                help="number of bases of the %s barcode (at least 1)" % where)
        parser.add_argument("--device", default=None, help="GPU index or torch device (default: current GPU)")
        parser.add_argument("--inflate", default=fastq.DEFAULT_INFLATE, choices=list(fastq.INFLATE_MODES),
                            help="who inflates BGZF-compressed FASTQ: auto = the GPU (any other file is read on the "
                                 "host), host = the host for every file")
        args = parser.parse_args(args) if args else parser.parse_args()
        cls._validate_barcode_args(args)
        tags = {"cell": (consts.QUALITY_CELL_BARCODE_TAG_KEY, consts.RAW_CELL_BARCODE_TAG_KEY),
                "molecule": (consts.QUALITY_MOLECULE_BARCODE_TAG_KEY, consts.RAW_MOLECULE_BARCODE_TAG_KEY),
                "sample": (consts.QUALITY_SAMPLE_BARCODE_TAG_KEY, consts.RAW_SAMPLE_BARCODE_TAG_KEY)}
        for name, (quality_tag, sequence_tag) in tags.items():
            start, length = getattr(args, name + "_barcode_start_pos"), getattr(args, name + "_barcode_length")
            if length:  # (set on the class and kept, as the reference does)
                setattr(cls, name + "_barcode", fastq.EmbeddedBarcode(start=start, end=start + length,
                                                                      quality_tag=quality_tag, sequence_tag=sequence_tag))
        cls._tag_bamfile(args.u2, args.output_bamfile, cls._make_tag_generators(args.r1, args.i1, args.whitelist),
                         device=args.device, inflate=args.inflate)
        return 0


COMMANDS = {
    "CalculateCellMetrics": GenericPlatform.calculate_cell_metrics,
    "CalculateGeneMetrics": GenericPlatform.calculate_gene_metrics,
    "MergeCellMetrics": GenericPlatform.merge_cell_metrics,
    "MergeGeneMetrics": GenericPlatform.merge_gene_metrics,
    "SplitBam": GenericPlatform.split_bam,
    "TagSortBam": GenericPlatform.tag_sort_bam,
    "VerifyBamSort": GenericPlatform.verify_bam_sort,
    "CreateCountMatrix": GenericPlatform.bam_to_count_matrix,
    "MergeCountMatrices": GenericPlatform.merge_count_matrices,
    "CorrectBarcodes": GenericPlatform.correct_barcodes,
    "Attach10xBarcodes": TenXV2.attach_barcodes,
    "AttachBarcodes": BarcodePlatform.attach_barcodes,
    "FastqMetrics": GenericPlatform.fastq_metrics,
    "FastqProcess": GenericPlatform.fastq_process,
    "FastqSlideseq": GenericPlatform.fastq_process,
    "TagSort": GenericPlatform.tag_sort,
}
