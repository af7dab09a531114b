"""hadoop_bam — MI355X-native BAM read path with Hadoop-BAM's input API.

Mirrors org.seqdoop.hadoop_bam.{BAMInputFormat, BAMRecordReader, FileVirtualSplit,
SAMRecordWritable, BAMSplitGuesser, util.BGZFSplitGuesser, util.BGZFBlockIndexer/BGZFBlockIndex/BGZFSplitFileInputFormat, SplittingBAMIndex, SplittingBAMIndexer}, the Sort plugin's
shuffle sort (cli/plugins/Sort) and its BAM output (BAMRecordWriter, KeyIgnoringBAMOutputFormat,
util.SAMOutputPreparer, cli.Utils.mergeSAMInto) and its SAM text output (SAMRecordWriter,
KeyIgnoringAnySAMOutputFormat, the View plugin), and the read formats FASTQ and QSEQ in both
directions (FastqInputFormat, QseqInputFormat, FastqOutputFormat, QseqOutputFormat), FASTA input
(FastaInputFormat, ReferenceFragment), and VCF text
output over BCF records (VCFRecordWriter, KeyIgnoringVCFOutputFormat, vcf_sort), and the summarize
and summarysort plugins (cli/plugins/chipster: SummarizeReducer, SummarizeOutputFormat); compute runs
in libhbam.so (HIP, gfx950) through the C ABI of include/hbam.h.
"""
from ._lib import Context, HbamUnavailable, load  # noqa: F401
from .formats import (  # noqa: F401
    AnySAMInputFormat, BAMInputFormat, BGZFBlockIndex, BGZFBlockIndexer, BGZFSplitFileInputFormat, BAMRecordReader, BAMSplitGuesser, BGZFSplitGuesser,
    Configuration, FileSplit, FileVirtualSplit, SAMRecordWritable, SplittingBAMIndex,
    SplittingBAMIndexer, compute_file_splits)
from .sort import HipSortOps, RcclComm, SortedRun, sort_sharded  # noqa: F401
from .output import (  # noqa: F401
    BAMRecordWriter, KeyIgnoringBAMOutputFormat, KeyIgnoringBAMRecordWriter, SAMFileHeader,
    SAMOutputPreparer, merge_sam_into, read_sam_header)
from .index import BAMIndex, BAMIndexer, IndexedBAMReader, parse_region  # noqa: F401
from .sam import (  # noqa: F401
    SAMFormat, SAMInputFormat, SAMRecordReader, SAMUnsupportedException, read_sam_text_header)
from .sam_text import (  # noqa: F401
    AnySAMOutputFormat, KeyIgnoringAnySAMOutputFormat, KeyIgnoringSAMRecordWriter, SAMRecordWriter,
    java_float_to_string, render_record, view)
from .fastq import (  # noqa: F401
    FastqInputFormat, FastqRecordReader, FormatConstants, FormatException, NumberFormatException,
    QseqInputFormat, QseqRecordReader, SequencedFragment)
from .fasta import FastaInputFormat, FastaRecordReader, ReferenceFragment  # noqa: F401
from .fastq_text import (  # noqa: F401
    FastqOutputFormat, FastqRecordWriter, QseqOutputFormat, QseqRecordWriter, convert)
from .summarize import (  # noqa: F401
    SummarizeOutputFormat, SummarizeReducer, SummaryGroup, getSummaryName, summarize, summary_sort)
from .vcf_text import (  # noqa: F401
    KeyIgnoringVCFOutputFormat, KeyIgnoringVCFRecordWriter, VCFHeader, VCFOutputFormat, VCFRecordWriter,
    VCFUnsupportedException, read_vcf_header_from)
