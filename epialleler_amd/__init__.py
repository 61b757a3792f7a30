"""epialleler_amd -- MI355X-native engine for epialleleR's per-read methylation-call
aggregation hot path (rcpp_threshold_reads / rcpp_get_xm_beta / rcpp_cx_report /
rcpp_mhl_report, rcpp_get_base_freqs for generateVcfReport, rcpp_call_methylation_genome for
callMethylation, rcpp_simulate_bam for simulateBam) behind the reference's own R-level interface.

Compute lives in csrc/ (hand-written HIP for gfx950 behind the C ABI of
include/epihip.h); this package is the host-side mirror of the R functions.
"""
from .api import (CONTEXT_TO_BASES, CONTEXT_LEVELS, FDRP_COLUMNS, GROUP_COMPARE_COLUMNS, GROUP_TESTS, MBIAS_COLUMNS, P_ADJUST_METHODS, REGION_COLUMNS, STRAND_LEVELS, ProcessedBam, Report, adjustPValues, adjustReport,  # noqa: F401
                  chisqPValues, compareCytosineGroups, compareCytosineReports, compareHeterogeneity, generateGroupDmrReport, rcpp_cx_compare_groups, tTestPValues,
                  cytosine_report_fused, fisherExact, generateAdjustedDmrReport, generateCytosineReport, generateDmrReport, generateFdrpReport, generateHaplotypeBlocks, generateHeterogeneityReport, generateLinkageReport,
                  generateMbiasReport, generateMhlReport, preprocessBam, rcpp_mbias_report, suggestTrim,
                  rcpp_cx_compare, rcpp_cx_compare_regions, rcpp_cx_report, rcpp_fdrp_report, rcpp_heterogeneity_compare, rcpp_heterogeneity_report, rcpp_linkage_blocks, rcpp_linkage_report,
                  rcpp_extract_patterns, rcpp_extract_patterns_multi, rcpp_get_xm_beta, rcpp_mhl_report, rcpp_region_report, rcpp_summarise_patterns_multi,
                  rcpp_threshold_reads, writeReport,
                  SMOOTH_COLUMNS, generateSmoothedReport, mergeCpgStrands, rcpp_cx_merge_strands, rcpp_cx_smooth, smoothCytosineReport,
                  EPI_SEGMENT_MAX_COVERAGE, EPI_SEGMENT_MAX_SITES, EPI_SEGMENT_MAX_STATES, EPI_SEGMENT_MIN_STATES, SEGMENT_COLUMNS, SEGMENT_SITE_COLUMNS,
                  generateSegmentReport, rcpp_cx_segment, segmentCytosineReport)
from .bed import (Bed, Ecdf, extractPatterns, extractPatternsBed, generateAmpliconReport, generateBedEcdf,  # noqa: F401
                  generateBedReport, generateCaptureReport, generateRegionReport, readBed, selectPatterns, summarisePatterns)
from .genome import Genome, callMethylation, preprocessGenome, rcpp_call_methylation_genome, rcpp_read_genome  # noqa: F401
from .simulate import rcpp_simulate_bam, simulateBam  # noqa: F401
from .vcf import (ASM_COLUMNS, ASM_SNV_COLUMNS, Vcf, allele_masks, generateAsmReport, generateAsmSnvReport, generateVcfReport,  # noqa: F401
                  rcpp_asm_report, rcpp_fep, rcpp_get_base_freqs, readVcf)
from ._lib import EpihipError  # noqa: F401
