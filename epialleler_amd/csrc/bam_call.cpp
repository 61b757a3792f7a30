// callMethylation: the call set both of its routes share (bam_call.hpp), and the BAM-to-BAM pipeline.
#include <sys/stat.h>
#include <unistd.h>
#include "bam_call.hpp"
#include "bam_device.hpp"

using namespace epi;
using namespace epi::bam;

namespace epi {
namespace bam {

// .callMethylation (R/internal.R:412-423): the strand tag from the first 1024 records; force_tag ("XG" / "YD" / "ZS")
// skips the look (rcpp_call_methylation_genome's own contract)
int call_choose_tag(const Rec *recs, size_t nrec, const char *force_tag, StrandTag *tag) {
  bool tXG = false, tYD = false, tZS = false;
  for (size_t i = 0; i < nrec && i < 1024; i++) {
    tXG |= aux_find(recs[i], 'X', 'G') != nullptr;
    tYD |= aux_find(recs[i], 'Y', 'D') != nullptr;
    tZS |= aux_find(recs[i], 'Z', 'S') != nullptr;
  }
  if (force_tag) *tag = strcmp(force_tag, "XG") == 0 ? TAG_XG : strcmp(force_tag, "YD") == 0 ? TAG_YD : TAG_ZS;
  else if (nrec == 0) return fail(EPI_ERR_ARG, "Empty file provided! Exiting");
  else if (tXG) *tag = TAG_XG;
  else if (tYD) *tag = TAG_YD;
  else if (tZS) *tag = TAG_ZS;
  else return fail(EPI_ERR_ARG, "Unable to call methylation: neither of XG/YD/ZS tags is present (genome strand unknown).\nExiting");
  return EPI_OK;
}

// the header's reference sequences must be the genome's, by name and length (src/rcpp_call_methylation.cpp:41-72)
int call_check_genome(epi_genome *g, const std::vector<std::string> &names, const std::vector<int64_t> &lens) {
  const int32_t ng = epi_genome_count(g);
  for (size_t i = 0; i < names.size(); i++)
    if ((int32_t)i >= ng || epi_genome_length(g, (int32_t)i) != lens[i] || names[i] != epi_genome_name(g, (int32_t)i))
      return fail(EPI_ERR_ARG, "BAM reference sequence doesn't match the provided genome sequence");
  return EPI_OK;
}

// Which of recs[0, n) are called (mapped, carrying the strand tag, no XM: :84-89), their strand letters (the tag's first
// two characters, or the strand YD / ZS names: :92-97), and the checks that keep every access in bounds (DESIGN.md
// section 2: the reference reads out of bounds here).  A called record grows by the XG tag (YD / ZS input) and XM.
int call_select(const Rec *recs, size_t n, StrandTag tag, const std::vector<std::string> &names,
                const std::vector<int64_t> &lens, size_t K, const char *who, CallSet &S) {
  const char t0 = tag == TAG_XG ? 'X' : tag == TAG_YD ? 'Y' : 'Z', t1 = tag == TAG_XG ? 'G' : tag == TAG_YD ? 'D' : 'S';
  S.call.resize(n); S.s_meth.resize(n); S.s_conv.resize(n);
  return parallel_ranges(K, n, who, [&](size_t lo, size_t hi) -> int {
    for (size_t i = lo; i < hi; i++) {
      const Rec &r = recs[i];
      S.call[i] = 0;
      const uint8_t *st = aux_find(r, t0, t1);
      if ((r.flag & 4) || !st || aux_find(r, 'X', 'M')) continue;          // written unchanged
      // the strand tag's first two characters (bam_aux_get's pointer [1] and [2])
      const uint8_t c1 = st + 1 < r.end ? st[1] : 0, c2 = st + 2 < r.end ? st[2] : 0;
      if (tag == TAG_XG) { S.s_meth[i] = c1; S.s_conv[i] = c2; }
      else {
        const bool ga = tag == TAG_YD ? c1 == 'r' : c1 == '-';
        S.s_meth[i] = ga ? 'G' : 'C'; S.s_conv[i] = ga ? 'A' : 'T';
      }
      if (r.tid < 0 || (size_t)r.tid >= names.size()) return fail(EPI_ERR_ARG, "corrupt BAM record %s: reference id out of range", r.qname);
      if (r.pos < 0) return fail(EPI_ERR_ARG, "corrupt BAM record %s: position out of range", r.qname);
      uint64_t qlen, rlen;
      bool bad_op;
      cigar_lens(r, &qlen, &rlen, &bad_op);
      if (bad_op) return fail(EPI_ERR_ARG, "Unknown CIGAR operation for BAM entry %s", r.qname);
      if (qlen != (uint64_t)r.l_seq) return fail(EPI_ERR_ARG, "corrupt BAM record %s: CIGAR does not match the sequence length", r.qname);
      if ((uint64_t)r.pos + rlen > (uint64_t)lens[(size_t)r.tid])
        return fail(EPI_ERR_ARG, "corrupt BAM record %s: alignment runs past the end of reference sequence %s", r.qname, names[(size_t)r.tid].c_str());
      const uint64_t bs = (uint64_t)(r.end - (const uint8_t *)r.qname) + 32;   // block_size (the name follows 32 fixed bytes)
      if (bs + (tag == TAG_XG ? 0 : 6) + 4 + (uint64_t)r.l_seq > 0x7FFFFFFFull)
        return fail(EPI_ERR_ARG, "corrupt BAM record %s: record too large", r.qname);
      S.call[i] = 1;
    }
    return EPI_OK;
  });
}

// the CallRec, CIGAR and SEQ inputs of the called records among recs[0, n) (n: at most call_select's range)
int call_pack_inputs(const Rec *recs, size_t n, size_t K, const char *who, CallSet &S) {
  S.call_idx.resize(n);
  S.crec.clear();
  int64_t ncig = 0, nseq = 0, nxm = 0;
  for (size_t i = 0; i < n; i++) {
    if (!S.call[i]) continue;
    const Rec &r = recs[i];
    CallRec c;
    memset(&c, 0, sizeof(c));
    c.cig_off = ncig; c.seq_off = nseq; c.xm_off = nxm;
    c.tid = r.tid; c.pos = r.pos; c.l_seq = r.l_seq; c.n_cig = (int32_t)r.n_cigar;
    c.s_meth = S.s_meth[i]; c.s_conv = S.s_conv[i];
    S.call_idx[i] = (int64_t)S.crec.size();
    S.crec.push_back(c);
    ncig += r.n_cigar; nseq += ((int64_t)r.l_seq + 1) / 2; nxm += r.l_seq;
  }
  S.ncig = ncig; S.nseq = nseq; S.nxm = nxm;
  S.cigar.resize((size_t)ncig); S.seq.resize((size_t)nseq); S.xm.resize((size_t)nxm);
  return parallel_ranges(K, n, who, [&](size_t lo, size_t hi) -> int {
    for (size_t i = lo; i < hi; i++) {
      if (!S.call[i]) continue;
      const Rec &r = recs[i];
      const CallRec &c = S.crec[(size_t)S.call_idx[i]];
      if (r.n_cigar) memcpy(S.cigar.data() + c.cig_off, r.cigar, 4 * (size_t)r.n_cigar);
      if (r.l_seq) memcpy(S.seq.data() + c.seq_off, r.seq, ((size_t)r.l_seq + 1) / 2);
    }
    return EPI_OK;
  });
}

}  // namespace bam
}  // namespace epi

namespace {

// ---- callMethylation: BAM in, BAM out (rcpp_call_methylation_genome, src/rcpp_call_methylation.cpp:27-177, with
// .callMethylation's tag choice, R/internal.R:405-432) ------------------------------------------------------------------
// The file goes through the reader's windows (block scan, parallel inflate and parse_record).  Per window the
// host picks the records to call (mapped, carrying the strand tag, no XM yet), checks them and packs their CIGAR and
// SEQ; the GPU computes their XM bytes (call_methylation.hip); the records are then written out in input order -- the
// called ones with XG (when the tag was YD or ZS) and XM appended -- and deflated into BGZF blocks by `nthreads`
// threads.  Host memory is bounded by the window (inflated bytes, the records written out, the packed call inputs).
struct Window {                       // what one window's records turn into
  std::vector<uint64_t> out_off;      // per record: where its output starts (n + 1 entries)
  std::vector<uint8_t> out;
};

// the window's records, in input order, with the new tags appended (bam_aux_append / bam_aux_update_str)
int call_splice(BamWindows &win, const CallSet &S, StrandTag tag, size_t K, Window &W) {
  const size_t nrec = win.recs.size();
  W.out.resize((size_t)W.out_off[nrec]);
  return parallel_ranges(K, nrec, "epi_call_methylation", [&](size_t lo, size_t hi) -> int {
    for (size_t i = lo; i < hi; i++) {
      const uint8_t *src = win.record(i);
      const uint32_t bs = rd32(src);
      uint8_t *o = W.out.data() + W.out_off[i];
      if (!S.call[i]) { memcpy(o, src, 4 + (size_t)bs); continue; }
      const uint64_t nb = W.out_off[i + 1] - W.out_off[i] - 4;
      o[0] = (uint8_t)nb; o[1] = (uint8_t)(nb >> 8); o[2] = (uint8_t)(nb >> 16); o[3] = (uint8_t)(nb >> 24);
      memcpy(o + 4, src + 4, bs);
      o += 4 + (size_t)bs;
      if (tag != TAG_XG) {
        const bool ga = S.s_meth[i] == 'G';
        const uint8_t xg[6] = {'X', 'G', 'Z', (uint8_t)(ga ? 'G' : 'C'), (uint8_t)(ga ? 'A' : 'T'), 0};
        memcpy(o, xg, 6);
        o += 6;
      }
      o[0] = 'X'; o[1] = 'M'; o[2] = 'Z';
      const Rec &r = win.recs[i];
      if (r.l_seq) memcpy(o + 3, S.xm.data() + S.crec[(size_t)S.call_idx[i]].xm_off, (size_t)r.l_seq);
      o[3 + r.l_seq] = 0;
    }
    return EPI_OK;
  });
}

int call_impl(epi_engine *eng, const char *in_path, const char *out_path, epi_genome *g, const char *force_tag,
              int nthreads, int32_t window_kib, int64_t *nrecs_out, int64_t *ncalled_out) {
  BamWindows win;
  EPI_TRY(win.open(in_path, window_kib, (size_t)64 << 20, nthreads, "Unable to read input BAM header"));
  const size_t K = thread_cap(nthreads);
  bool checked = false;
  StrandTag tag = TAG_XG;
  BgzfWriter out;
  DeviceStatePtr dev = device_state_new();
  CallSet S;
  Window W;
  int64_t nrecs = 0, ncalled = 0;
  // phase times (EPIHIP_BAM_TIMING, as for the reader): inflate + index, host preparation, GPU, splice, deflate + write
  const bool timing = epi::options().bam_timing != 0;
  double t_phase[5] = {0, 0, 0, 0, 0}, t_mark = tnow();
  auto lap = [&](int k) { const double t = tnow(); t_phase[k] += t - t_mark; t_mark = t; };

  for (;;) {
    bool final;
    EPI_TRY(win.next(&final));
    const Rec *recs = win.recs.begin();
    const size_t nrec = win.recs.size();
    lap(0);
    if (!checked) {
      if (nrec < 1024 && !final) { win.keep_all(); continue; }   // .checkBam looks at the first 1024 records
      EPI_TRY(call_choose_tag(recs, nrec, force_tag, &tag));
      // ---- the output and the header check (src/rcpp_call_methylation.cpp:41-72) ----
      EPI_TRY(out.open(out_path));
      EPI_TRY(call_check_genome(g, win.names, win.lens));
      EPI_TRY(out.write(win.header(), win.header_size(), nthreads));   // the input header, verbatim
      checked = true;
    }
    // ---- which records are called, and how large each one is written out ----
    EPI_TRY(call_select(recs, nrec, tag, win.names, win.lens, K, "epi_call_methylation", S));
    W.out_off.resize(nrec + 1);
    W.out_off[0] = 0;
    for (size_t i = 0; i < nrec; i++) {
      const uint64_t bs = rd32(win.record(i));
      W.out_off[i + 1] = W.out_off[i] + 4 + bs + (S.call[i] ? (tag == TAG_XG ? 0 : 6) + 4 + (uint64_t)recs[i].l_seq : 0);
    }
    // ---- the packed inputs of the called records ----
    EPI_TRY(call_pack_inputs(recs, nrec, K, "epi_call_methylation", S));
    const int64_t ncall = (int64_t)S.crec.size();
    lap(1);
    // ---- the GPU: XM of every called record ----
    EPI_TRY(device_call_window(dev.get(), eng, g, S.crec.data(), ncall, S.cigar.data(), S.ncig, S.seq.data(), S.nseq, S.nxm,
                               CALL_XM, S.xm.data()));
    lap(2);
    EPI_TRY(call_splice(win, S, tag, K, W));
    lap(3);
    EPI_TRY(out.write(W.out.data(), W.out.size(), nthreads));
    lap(4);
    nrecs += (int64_t)nrec;
    ncalled += ncall;
    win.consume(nrec);
    if (final) break;
  }
  if (!checked) return fail(EPI_ERR_ARG, "Empty file provided! Exiting");
  EPI_TRY(out.close());
  lap(4);
  if (timing)
    fprintf(stderr, "[call] inflate+index %.3f s  prepare %.3f s  gpu %.3f s  splice %.3f s  deflate+write %.3f s\n",
            t_phase[0], t_phase[1], t_phase[2], t_phase[3], t_phase[4]);
  *nrecs_out = nrecs;
  *ncalled_out = ncalled;
  return EPI_OK;
}

}  // namespace

extern "C" {

int epi_call_methylation_windowed(epi_engine *eng, const char *in_path, const char *out_path, epi_genome *g, const char *tag,
                                  int nthreads, int32_t window_kib, int64_t *nrecs, int64_t *ncalled) {
  if (!in_path || !out_path || !g || !nrecs || !ncalled) return fail(EPI_ERR_ARG, "epi_call_methylation: NULL argument");
  if (tag && strcmp(tag, "XG") != 0 && strcmp(tag, "YD") != 0 && strcmp(tag, "ZS") != 0)
    return fail(EPI_ERR_ARG, "epi_call_methylation: tag must be XG, YD or ZS");
  *nrecs = 0; *ncalled = 0;
  EPI_TRY(device_engine(&eng, "epi_call_methylation: the calls are made on the GPU"));   // no device: fails here, before any file is touched
  int rc;
  bool wrote = false;
  try {
    struct stat st;
    wrote = !(*out_path && stat(out_path, &st) == 0);        // (a partial output is removed only if this call created it)
    rc = call_impl(eng, in_path, out_path, g, tag, nthreads, window_kib, nrecs, ncalled);
  } catch (const std::bad_alloc &) {
    rc = fail(EPI_ERR_NOMEM, "epi_call_methylation: out of host memory");
  } catch (...) {
    rc = fail(EPI_ERR_ARG, "epi_call_methylation: unexpected failure while reading %s", in_path);
  }
  if (rc != EPI_OK) {
    *nrecs = 0; *ncalled = 0;
    if (wrote && *out_path) (void)unlink(out_path);
  }
  return rc;
}

int epi_call_methylation(epi_engine *eng, const char *in_path, const char *out_path, epi_genome *g, int nthreads,
                         int64_t *nrecs, int64_t *ncalled) {
  return epi_call_methylation_windowed(eng, in_path, out_path, g, nullptr, nthreads, 0, nrecs, ncalled);
}

}  // extern "C"
