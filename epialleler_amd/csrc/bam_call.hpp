// callMethylation's call set (rcpp_call_methylation_genome, src/rcpp_call_methylation.cpp:27-177, with
// .callMethylation's tag choice, R/internal.R:405-432): which records are called and what the GPU needs for them.
// Shared by callMethylation (BAM out, call_impl in bam_call.cpp) and preprocessBam with a genome (preprocess_impl in
// bam_pack.cpp), so that the second sees exactly the records, strand letters and errors the first would have produced.
// Pure host code.
#pragma once
#include "bam_reader.hpp"

namespace epi {
namespace bam {

enum StrandTag { TAG_XG = 0, TAG_YD = 1, TAG_ZS = 2 };

struct CallSet {                      // the records of one window to call
  std::vector<uint8_t> call;          // per record: 1 = call it
  std::vector<uint8_t> s_meth, s_conv;
  std::vector<int64_t> call_idx;      // per called record of the packed range: its index among the called ones
  std::vector<CallRec> crec;
  std::vector<uint32_t> cigar;
  std::vector<uint8_t> seq;
  std::vector<uint8_t> xm;            // the GPU's output: l_seq bytes per called record, at its xm_off
  int64_t ncig = 0, nseq = 0, nxm = 0;
};

// (bam_call.cpp has the rules each one restates)
// the strand tag from the first 1024 records, or force_tag ("XG" / "YD" / "ZS")
int call_choose_tag(const Rec *recs, size_t nrec, const char *force_tag, StrandTag *tag);
// the header's reference sequences must be the genome's, by name and length
int call_check_genome(epi_genome *g, const std::vector<std::string> &names, const std::vector<int64_t> &lens);
// which of recs[0, n) are called, their strand letters, and the checks that keep every access in bounds; K threads
int call_select(const Rec *recs, size_t n, StrandTag tag, const std::vector<std::string> &names,
                const std::vector<int64_t> &lens, size_t K, const char *who, CallSet &S);
// the CallRec, CIGAR and SEQ inputs of the called records among recs[0, n) (n: at most call_select's range)
int call_pack_inputs(const Rec *recs, size_t n, size_t K, const char *who, CallSet &S);

}  // namespace bam
}  // namespace epi
