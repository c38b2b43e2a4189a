"""MI355X-native k-mer spectrum builder (Kmernator FilterReads / KmerSpectrum hot path).

Everything that computes lives in csrc/ (hand-written HIP for gfx950 behind the C-ABI of
include/kmernator_amd.h); this package is the thin host-side mirror of the reference's
KmerSpectrum interface plus the one-process-per-GPU owner-partitioned driver.
"""
from ._lib import (KMR_MAP_SINGLETON, KMR_MAP_WEAK, KMR_VALUE_COUNT_DIR, KMR_VALUE_EXT, KmrArtifactReportConfig, KmrCompareCounts, KmrConfig, KmrDedupConfig, KmrExtendConfig, KmrExtendStop, KmrMatchConfig, KmrNormalizeConfig, KmrPartitionConfig, KmrSelectConfig, KmrTnfLikelihoodConfig, KMR_TNF_EUCLIDEAN, KMR_TNF_SPEARMAN, default_config, load,
                   record_bytes)
from .spectrum import COMPARE_DTYPE, COMPARE_HEADER, CompareSpectrums, ConsensusReadSet, ContigExtender, DedupPass, EXTEND_STOP_DTYPE, ExtendResults, ExtendRound, DumpText, DuplicateFragmentFilter, FilterKnownOddities, FilterReport, KmerMatch, KmerSpectrum, KmerSpectrumError, Histogram, MatchResults, ReadPairs, ReadSelector, ReadSet, TnfDistance, TnfVectors, compare_line, extendContigsWithContigExtender, finishLongContigs, synth_reads_device, tnf_columns, tnf_dims, tnf_header

__all__ = ["KmerSpectrum", "DumpText", "KmerSpectrumError", "ReadSet", "ReadPairs", "Histogram", "FilterKnownOddities", "FilterReport", "DuplicateFragmentFilter", "DedupPass", "ConsensusReadSet", "ReadSelector", "synth_reads_device", "CompareSpectrums", "compare_line", "KmerMatch", "MatchResults", "KmrMatchConfig", "ContigExtender", "ExtendResults", "ExtendRound", "EXTEND_STOP_DTYPE", "extendContigsWithContigExtender", "finishLongContigs", "KmrExtendConfig", "KmrExtendStop", "TnfDistance", "TnfVectors", "tnf_dims", "tnf_columns", "tnf_header", "KmrTnfLikelihoodConfig", "KMR_TNF_EUCLIDEAN", "KMR_TNF_SPEARMAN", "COMPARE_DTYPE", "COMPARE_HEADER", "KmrCompareCounts", "KmrConfig", "KmrSelectConfig", "KmrPartitionConfig", "KmrNormalizeConfig", "KmrDedupConfig", "KmrArtifactReportConfig", "default_config", "load", "record_bytes",
           "KMR_MAP_WEAK", "KMR_MAP_SINGLETON", "KMR_VALUE_COUNT_DIR", "KMR_VALUE_EXT"]
