"""lofreq_amd -- MI355X-native implementation of LoFreq's per-pileup-column SNV calling path.

Scope: plp_to_errprobs -> snpcaller/poissbin/pruned_calc_prob_dist ->
Bonferroni emit test, behind LoFreq's column interface.  Compute lives in hand-written HIP kernels
(lofreq_amd/csrc, gfx950) behind the C ABI of include/lofreq_amd.h; this package is the thin host
mirror of the reference interface plus region sharding across GPUs.
"""
from ._lib import (LFQ_BAM_DROP_ALN_TAGS, LFQ_BAM_KEEP_EXISTING, LFQ_BAM_PUT_ALIGNMENT, LFQ_BAM_PUT_IDAQ, LFQ_BAM_PUT_INDELQUAL,
                   LFQ_BAM_PUT_LB, LFQ_BAM_READ_IDAQ, LFQ_BAM_READ_LB, LFQ_BGZF_PUT_EOF)
from ._lib import (COL_COUNTS_DTYPE, COL_PVALS_DTYPE, SNV_RECORD_DTYPE, LFQ_PV_LOG, LFQ_PV_LOG_FECLAMP,
                   LFQ_PV_NONE, LFQ_PV_UNDERFLOW, LFQ_USE_BAQ, LFQ_USE_IDAQ, LFQ_USE_MQ, LFQ_USE_SQ,
                   INDEL_RECORD_DTYPE)
from .caller import (PileupBatch, SnvCaller, VarcallConf, filter_records, finalize_pvals, format_vcf,
                     format_vcf_record,
                     pvalue_from_log, snvqual_thresh, write_vcf_header, binom_cdf, uniq_mtc)
from .baq import baq_batch, encode_seq
from .viterbi import viterbi_batch
from .indelqual import indelqual_batch
from .pileup import (DeviceTracks, PlpQuals, PlpSummary, ReadSet, format_plp_indel_quals, format_plp_quals,
                     format_plp_summary, last_bam_decode_times, last_bam_encode_times, last_baq_fill_stats, last_plp_quals_times, pileup_indel_columns, pileup_snv_tracks, plp_quals,
                     skip_snv_columns, BgzfError, bam_scan_records, bgzf_inflate, last_bgzf_times,
                     bam_frame_encoded, bgzf_deflate, last_bgzf_deflate_times)
from .bamindex import BamIndex, BamIndexError, bam_index_build, bam_record_chain, bam_record_cuts, last_bam_index_times
from .bed import Bed, BedError
from .fasta import Contig, Fasta, FastaError, FastaIndex, bgzf_gzi, bgzf_inflate_view, checkref, last_fasta_times
from .vcf import Vcf, VcfError, VcfIndex, last_vcf_index_times, last_vcf_times, vcf_write_gz, vcfset
from .srcq import source_qual_batch
from .indel import IndelColumns, call_indels, filter_indel_records, format_indel_record

__all__ = [
    "COL_COUNTS_DTYPE", "COL_PVALS_DTYPE", "SNV_RECORD_DTYPE", "LFQ_PV_LOG", "LFQ_PV_LOG_FECLAMP",
    "LFQ_PV_NONE", "LFQ_PV_UNDERFLOW", "LFQ_USE_BAQ", "LFQ_USE_MQ", "LFQ_USE_SQ", "PileupBatch", "SnvCaller", "VarcallConf",
    "filter_records", "finalize_pvals", "format_vcf", "format_vcf_record", "pvalue_from_log", "snvqual_thresh",
    "write_vcf_header", "LFQ_USE_IDAQ", "INDEL_RECORD_DTYPE", "IndelColumns", "call_indels", "format_indel_record", "filter_indel_records", "baq_batch", "viterbi_batch", "indelqual_batch", "encode_seq", "DeviceTracks", "pileup_snv_tracks",
    "source_qual_batch", "pileup_indel_columns", "skip_snv_columns", "ReadSet", "binom_cdf", "uniq_mtc",
    "PlpSummary", "format_plp_summary",
    "PlpQuals", "plp_quals", "format_plp_quals", "format_plp_indel_quals", "last_plp_quals_times",
    "last_bam_decode_times",
    "last_bam_encode_times", "LFQ_BAM_PUT_ALIGNMENT", "LFQ_BAM_DROP_ALN_TAGS", "LFQ_BAM_PUT_LB", "LFQ_BAM_PUT_IDAQ",
    "LFQ_BAM_KEEP_EXISTING", "LFQ_BAM_PUT_INDELQUAL",
    "LFQ_BAM_READ_LB", "LFQ_BAM_READ_IDAQ", "last_baq_fill_stats",
    "bgzf_inflate", "BgzfError", "bam_scan_records", "last_bgzf_times",
    "bgzf_deflate", "last_bgzf_deflate_times", "bam_frame_encoded", "LFQ_BGZF_PUT_EOF",
    "BamIndex", "BamIndexError", "bam_index_build", "last_bam_index_times", "bam_record_chain", "bam_record_cuts",
    "Bed", "BedError",
    "Fasta", "FastaIndex", "FastaError", "Contig", "checkref", "bgzf_gzi", "bgzf_inflate_view", "last_fasta_times",
    "Vcf", "VcfError", "vcfset", "last_vcf_times", "VcfIndex", "last_vcf_index_times", "vcf_write_gz",
]
