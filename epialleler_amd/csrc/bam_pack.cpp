// Host-side producer: BAM file -> sorted, packed SoA templates in pinned host memory.
//
// Replaces the reference's
//   rcpp_check_bam            src/rcpp_check_bam.cpp:19-60   + .checkBam  R/internal.R:75-128
//   rcpp_read_bam_paired      src/rcpp_read_bam.cpp:19-192   (short-read XG/XM alignments)
//   rcpp_read_bam_single      src/rcpp_read_bam.cpp:199-343
//   rcpp_read_bam_mm_single   src/rcpp_read_bam.cpp:364-579  (long-read MM/ML alignments: pack_mm below)
//   .readBam (templid, sort)  R/internal.R:154-199
// without HTSlib: the file comes as windows of parsed records from the reader (bam_reader.hpp), the records
// callMethylation would call from bam_call.hpp, and what runs on the device goes through bam_device.hpp.  The packed
// byte per reference position is (nt16 << 4) | ctx_to_idx(XM) (src/epialleleR.h:28-35), filler 0xFB (N,'-').
// Output is what the GPU engine consumes: one contiguous byte stream in (rname,start)
// order + offsets + int32 columns, page-locked when a HIP device is usable (so it can be
// streamed to HBM with hipMemcpyAsync) and from malloc otherwise.
#include <stdio.h>
#include <limits.h>
#include <algorithm>
#include <deque>
#include <numeric>
#include "bam_reader.hpp"
#include "bam_call.hpp"
#include "bam_device.hpp"

using namespace epi;
using namespace epi::bam;

namespace {

inline uint8_t ctx_idx(char c) { return (uint8_t)ctx_to_idx((unsigned char)c); }
inline uint8_t seqi_shifted(const uint8_t *s, uint32_t i) { return (uint8_t)((s[i >> 1] << ((i & 1) << 2)) & 0xF0); }   // epialleleR.h:32

// ---- long-read (MM/ML) records -------------------------------------------------------------------------------
// The reference leaves the MM/ML tags to HTSlib (bam_parse_basemod / bam_next_basemod; Rhtslib, version not pinned in
// DESCRIPTION).  HTSlib is not part of the reference tree, so this restates the published rules of the SAM tags
// specification (SAMtags.pdf section 1.7 "Base modifications"):
//   MM:Z:  ([ACGTUN][-+]([a-z]+|[0-9]+)[.?]?(,[0-9]+)*;)*   one entry per (canonical base, strand, modification codes);
//          each number = how many bases of that canonical type to skip before the next modified one, counted along
//          the read AS SEQUENCED: for a reverse-strand alignment from the end of SEQ, on the complemented base;
//          base N counts every base; several one-letter codes in one entry share the positions.
//   ML:B:C one probability (0..255) per listed position and code, in MM order, codes of an entry interleaved per
//          position.  Without ML the probability is unknown (-1, as HTSlib reports it).
// A ChEBI number n is carried as code -n (HTSlib's convention, which rcpp_read_bam.cpp:474 relies on for 27551).
struct ModHit { int32_t pos; int32_t code; int32_t strand; int32_t qual; };

inline int nt16_of(char c) {
  switch (c) { case 'A': return 1; case 'C': return 2; case 'G': return 4; case 'T': case 'U': return 8; case 'N': return 15; default: return -1; }
}
inline int nt16_complement(int c) { return c == 1 ? 8 : c == 8 ? 1 : c == 2 ? 4 : c == 4 ? 2 : c; }
inline int seqi(const uint8_t *s, uint32_t i) { return (s[i >> 1] >> ((~i & 1) << 2)) & 0xF; }

void parse_basemods(const Rec &r, const char *mm, bool has_ml, const uint8_t *ml, uint32_t n_ml, std::vector<ModHit> &hits) {
  hits.clear();
  const bool rev = (r.flag & 16) != 0;
  const int32_t L = r.l_seq;
  uint32_t ml_idx = 0;
  const char *p = mm;
  while (*p) {
    const int base = nt16_of(*p);
    if (base < 0) return;                                        // malformed: HTSlib gives up on the tag
    p++;
    if (*p != '+' && *p != '-') return;
    const int32_t strand = *p == '-' ? 1 : 0;
    p++;
    int32_t codes[16];
    int ncodes = 0;
    if (*p >= '0' && *p <= '9') {                                // one ChEBI number
      long v = 0;
      while (*p >= '0' && *p <= '9') { v = v * 10 + (*p - '0'); p++; }
      codes[ncodes++] = (int32_t)-v;
    } else {
      while (*p >= 'a' && *p <= 'z') { if (ncodes < 16) codes[ncodes++] = (int32_t)*p; p++; }
    }
    if (ncodes == 0) return;
    if (*p == '.' || *p == '?') p++;                             // implicit / explicit mode: only listed bases matter here
    const int target = rev ? nt16_complement(base) : base;
    int32_t i = rev ? L - 1 : 0;                                 // next base of SEQ to look at, in sequencing order
    const int32_t step = rev ? -1 : 1;
    while (*p == ',') {
      p++;
      long skip = 0;
      if (!(*p >= '0' && *p <= '9')) return;
      while (*p >= '0' && *p <= '9') { skip = skip * 10 + (*p - '0'); p++; }
      // advance to the (skip+1)-th base of the canonical type
      int32_t found = -1;
      while (i >= 0 && i < L) {
        const bool match = target == 15 || seqi(r.seq, (uint32_t)i) == target;
        const int32_t at = i;
        i += step;
        if (match) { if (skip == 0) { found = at; break; } skip--; }
      }
      if (found < 0) return;                                     // the tag points beyond the sequence
      for (int k = 0; k < ncodes; k++) {
        ModHit h;
        h.pos = found; h.code = codes[k]; h.strand = strand;
        h.qual = has_ml ? (ml_idx < n_ml ? (int32_t)ml[ml_idx] : -1) : -1;
        ml_idx++;
        hits.push_back(h);
      }
    }
    if (*p != ';') return;
    p++;
  }
}

// cytosine context of query base i from the base and its two neighbours, keyed like the reference's 512-entry tables
// (src/epialleleR.h:43-116) by the low three bits of the IUPAC letters: A=1 C=3 T=4 N=6 G=7, anything else gives '.'
inline bool tri_ok(int c) { return c == 1 || c == 3 || c == 4 || c == 6 || c == 7; }
inline char ctx_forward(int b0, int b1, int b2) {                // C at i: CG -> z, CHG -> x, CHH -> h
  if (b0 != 3 || !tri_ok(b1) || !tri_ok(b2)) return '.';
  return b1 == 7 ? 'z' : b2 == 7 ? 'x' : 'h';
}
inline char ctx_reverse(int b0, int b1, int b2) {                // G at i with (i-2, i-1, i): CG -> z, CHG -> x, CHH -> h
  if (b2 != 7 || !tri_ok(b0) || !tri_ok(b1)) return '.';
  return b1 == 3 ? 'z' : b0 == 3 ? 'x' : 'h';
}

// big_malloc as a standard allocator, for the packed bytes of a thread.  (Here and not next to big_malloc: with a type of
// this unit's own for its allocator the vector's members have internal linkage, and push_row's insert is inlined.)
template <class T> struct BigAlloc {
  using value_type = T;
  BigAlloc() = default;
  template <class U> BigAlloc(const BigAlloc<U> &) {}
  T *allocate(size_t n) { void *p = big_malloc(n * sizeof(T)); if (!p) throw std::bad_alloc(); return static_cast<T *>(p); }
  void deallocate(T *p, size_t) { free(p); }
  template <class U> bool operator==(const BigAlloc<U> &) const { return true; }
  template <class U> bool operator!=(const BigAlloc<U> &) const { return false; }
};

struct Packed {
  std::vector<int32_t> rname, strand, start;
  std::vector<int64_t> off;          // template t owns bytes [off[t], off[t+1])
  std::vector<uint8_t, BigAlloc<uint8_t>> bytes;
  // one template: 1-based rname and start, and row[0, width) less both trims (src/rcpp_read_bam.cpp:61-69, 303-306,
  // 537-541)
  void push_row(int32_t tid, int32_t strand_, int32_t pos, const uint8_t *row, int width, int trim5, int trim3) {
    rname.push_back(tid + 1);
    strand.push_back(strand_);
    start.push_back(pos + trim5 + 1);
    const int keep = width - (trim5 + trim3);
    if (keep > 0) bytes.insert(bytes.end(), row + trim5, row + trim5 + keep);
    off.push_back((int64_t)bytes.size());
  }
};

// (nt16 << 4) | ctx_idx(XM) of every query base of a record (src/epialleleR.h:28,32): two bases per byte of SEQ
inline void pack_query(const Rec &r, const char *xm, uint8_t *__restrict__ o) {
  const size_t n = (size_t)r.l_seq;
  const uint8_t *__restrict__ s = r.seq;
  const unsigned char *__restrict__ x = reinterpret_cast<const unsigned char *>(xm);
  for (size_t i = 0; i + 1 < n; i += 2) {
    const uint8_t b = s[i >> 1];
    o[i] = (uint8_t)((b & 0xF0) | (((x[i] + 2u) >> 2) & 15u));
    o[i + 1] = (uint8_t)(((b << 4) & 0xF0) | (((x[i + 1] + 2u) >> 2) & 15u));
  }
  if (n & 1) o[n - 1] = (uint8_t)((s[(n - 1) >> 1] & 0xF0) | (((x[n - 1] + 2u) >> 2) & 15u));
}
inline void packed_bytes(const Rec &r, const char *xm, std::vector<uint8_t> &pb) {
  pb.resize((size_t)r.l_seq + 2);
  pack_query(r, xm, pb.data());
}

// walk the CIGAR of one record into the template buffers; returns the reference position after the last op
template <class F>
int apply_cigar(const Rec &r, uint32_t dest0, F &&on_match, uint32_t *dest_end) {
  uint32_t qpos = 0, dpos = dest0;
  for (uint32_t i = 0; i < r.n_cigar; i++) {
    const uint32_t c = rd32(r.cigar + 4 * i), op = c & 0xF, len = c >> 4;
    switch (op) {
      case 0: case 7: case 8: on_match(qpos, dpos, len); qpos += len; dpos += len; break;    // M = X
      case 1: case 4: qpos += len; break;                                                     // I S
      case 2: case 3: dpos += len; break;                                                     // D N
      case 5: case 6: case 9: break;                                                          // H P B
      default: return fail(EPI_ERR_ARG, "Unknown CIGAR operation for BAM entry %s", r.qname);
    }
  }
  *dest_end = dpos;
  return EPI_OK;
}

// QNAME -> template id (mates = "anywhere"), ids given in the order the keys are first added.  Open addressing over a
// power-of-two table with the exact string compare; the keys are kept back to back (NUL-terminated), which also names
// the template in messages after its records' window is gone.
class QnameMap {
 public:
  static uint64_t hash(const char *q) {                      // FNV-1a, finalised
    uint64_t h = 0xCBF29CE484222325ull;
    for (; *q; q++) h = (h ^ (uint8_t)*q) * 0x100000001B3ull;
    return mix64(h);
  }
  uint32_t find_or_add(const char *q, uint64_t h) {
    if (2 * (hash_.size() + 1) > slot_.size()) grow();
    const size_t mask = slot_.size() - 1;
    size_t i = (size_t)h & mask;
    for (; slot_[i]; i = (i + 1) & mask) {
      const uint32_t g = slot_[i] - 1;
      if (hash_[g] == h && strcmp(name(g), q) == 0) return g;
    }
    const uint32_t g = (uint32_t)hash_.size();
    slot_[i] = g + 1;
    hash_.push_back(h);
    off_.push_back(names_.size());
    names_.insert(names_.end(), q, q + strlen(q) + 1);
    return g;
  }
  const char *name(uint32_t g) const { return names_.data() + off_[g]; }
  size_t size() const { return hash_.size(); }

 private:
  void grow() {
    slot_.assign(slot_.empty() ? 4096 : 2 * slot_.size(), 0u);
    const size_t mask = slot_.size() - 1;
    for (uint32_t g = 0; g < (uint32_t)hash_.size(); g++) {
      size_t i = (size_t)hash_[g] & mask;
      while (slot_[i]) i = (i + 1) & mask;
      slot_[i] = g + 1;
    }
  }
  std::vector<uint32_t> slot_;     // id + 1, 0: empty
  std::vector<uint64_t> hash_;     // per id
  std::vector<size_t> off_;        // per id: its key in names_
  std::vector<char> names_;
};

// ---- .readBam: skip flags (R/internal.R:173-177) and the packers ----
struct PackCtx {                      // what the packers read of the call's options and of the file; never written by them
  uint16_t skip_flags;
  int32_t min_mapq, min_baseq, min_prob, highest_prob, trim5, trim3;
  size_t n_ref;                       // the header's reference sequences
  const CallSet *calls;               // with a genome: the window's records called on the way in, else NULL
};

// XG's first letter and the XM bytes of record ri, as the packers see them: from its own tags, or -- a record called on
// the way in (genome) -- as callMethylation would have written it: its own XG, else the appended one (s_meth), and the
// appended XM, here the packed bytes the GPU made (*pcall).  false: not usable (no XG / XM string).
bool xg_xm(const PackCtx &c, size_t ri, const Rec &r, char *s, const char **xm, const uint8_t **pcall) {
  bool pg, pm;
  const char *xg = aux_z(r, 'X', 'G', &pg);
  *xm = nullptr; *pcall = nullptr;
  if (c.calls && c.calls->call[ri]) {
    if (!aux_clean(r) || (pg && !xg)) return false;         // (the appended tags cannot be reached / XG is not a string)
    *s = pg ? xg[0] : (char)c.calls->s_meth[ri];
    *pcall = c.calls->xm.data() + c.calls->crec[(size_t)c.calls->call_idx[ri]].xm_off;
    return true;
  }
  *xm = aux_z(r, 'X', 'M', &pm);
  if (!pg || !pm || !xg || !*xm) return false;
  *s = xg[0];
  return true;
}

// a record that enters a template must be self-consistent: the CIGAR consumes exactly the stored bases, XM covers
// them, the reference id exists (HTSlib rejects such records while reading; without the checks they index past
// the record).  *width: the reference bases the CIGAR spans (bam_cigar2rlen).
int use_record(const PackCtx &c, const Rec &r, const char *xm, uint32_t *width) {
  if (r.tid < 0 || (size_t)r.tid >= c.n_ref) return fail(EPI_ERR_ARG, "corrupt BAM record %s: reference id out of range", r.qname);
  uint64_t qlen, rlen;
  bool bad_op;                                              // (left to apply_cigar, which names it after these checks)
  cigar_lens(r, &qlen, &rlen, &bad_op);
  if (qlen != (uint64_t)r.l_seq) return fail(EPI_ERR_ARG, "corrupt BAM record %s: CIGAR does not match the sequence length", r.qname);
  if (xm && strlen(xm) < (size_t)r.l_seq) return fail(EPI_ERR_ARG, "corrupt BAM record %s: XM tag shorter than the sequence", r.qname);
  *width = (uint32_t)rlen;
  return EPI_OK;
}

// Each packer turns records [r_lo, r_hi) into templates appended to P; ranges are packed by several threads and
// concatenated in order (a paired-end range never starts inside a template).
int pack_mm(const PackCtx &c, const Rec *recs, size_t r_lo, size_t r_hi, Packed &P) {
  // ---- rcpp_read_bam_mm_single (src/rcpp_read_bam.cpp:364-579) ----
  static const char nt16_str[] = "=ACMGRSVTWYHKDBN";
  std::vector<char> seq, xm[2];
  std::vector<uint8_t> rs[2];
  std::vector<ModHit> hits;
  for (size_t ri = r_lo; ri < r_hi; ri++) {
    const Rec &r = recs[ri];
    if ((r.flag & c.skip_flags) || (int)r.mapq < c.min_mapq) continue;                        // :423-424
    uint32_t width;                                                                           // bam_cigar2rlen, :437
    EPI_TRY(use_record(c, r, nullptr, &width));
    const int record_strand = (r.flag & 16) ? 1 : 0;                                          // :426
    const int32_t qw = r.l_seq < 0 ? -r.l_seq : r.l_seq;                                      // :436
    rs[0].assign(width, 0xFB); rs[1].assign(width, 0xFB);                                     // :453-454
    seq.assign((size_t)qw + 4, 'N');                                                          // :457-461 NN + SEQ + NN
    for (int32_t i = 0; i < qw; i++) seq[(size_t)i + 2] = nt16_str[seqi(r.seq, (uint32_t)i)];
    xm[0].resize((size_t)qw); xm[1].resize((size_t)qw);
    for (int32_t i = 0; i < qw; i++) {                                                        // :464-467
      xm[0][(size_t)i] = ctx_forward(seq[(size_t)i + 2] & 7, seq[(size_t)i + 3] & 7, seq[(size_t)i + 4] & 7);
      xm[1][(size_t)i] = ctx_reverse(seq[(size_t)i] & 7, seq[(size_t)i + 1] & 7, seq[(size_t)i + 2] & 7);
    }
    bool strand_has_mods[2] = {false, false};
    bool pmm = false;
    const char *mm = aux_z(r, 'M', 'M', &pmm);
    if (!mm) mm = aux_z(r, 'M', 'm', &pmm);
    if (mm) {
      char sub = 0; uint32_t n_ml = 0; const uint8_t *ml = nullptr;
      bool has_ml = aux_b(r, 'M', 'L', &sub, &n_ml, &ml) || aux_b(r, 'M', 'l', &sub, &n_ml, &ml);
      if (has_ml && sub != 'C' && sub != 'c') has_ml = false;
      parse_basemods(r, mm, has_ml, ml, n_ml, hits);
      std::stable_sort(hits.begin(), hits.end(), [](const ModHit &x, const ModHit &y) { return x.pos < y.pos; });
      for (size_t a0 = 0; a0 < hits.size();) {                                                // one query position at a time, :469
        size_t a1 = a0;
        int ismeth[2] = {0, 0}, meth_prob[2] = {-2, -2}, max_other[2] = {-2, -2};             // :470-472
        for (; a1 < hits.size() && hits[a1].pos == hits[a0].pos; a1++) {
          const ModHit &h = hits[a1];
          if (h.code == 'm' || h.code == -27551) { ismeth[h.strand] = 1; meth_prob[h.strand] = h.qual; }   // :474-476
          else if (max_other[h.strand] < h.qual) max_other[h.strand] = h.qual;                             // :477-479
        }
        const int32_t mod_pos = hits[a0].pos;
        for (int sidx = 0; sidx < 2; sidx++) {                                                // :481-490
          const int cs = record_strand > sidx ? record_strand - sidx : sidx - record_strand;
          if (ismeth[sidx] && meth_prob[sidx] >= c.min_prob && (!c.highest_prob || meth_prob[sidx] > max_other[sidx]) &&
              xm[cs][(size_t)mod_pos] > 'A') {
            xm[cs][(size_t)mod_pos] &= (char)0xDF;
            strand_has_mods[cs] = true;
          }
        }
        a0 = a1;
      }
    }
    uint32_t dest_end = 0;
    EPI_TRY(apply_cigar(r, 0, [&](uint32_t qpos, uint32_t dpos, uint32_t len) {              // :494-531
      for (uint32_t j = 0; j < len; j++)
        if ((int)r.qual[qpos + j] >= c.min_baseq) {
          const uint8_t hi = seqi_shifted(r.seq, qpos + j);
          rs[0][dpos + j] = (uint8_t)(hi | ctx_idx(xm[0][qpos + j]));
          rs[1][dpos + j] = (uint8_t)(hi | ctx_idx(xm[1][qpos + j]));
        }
    }, &dest_end));
    strand_has_mods[record_strand] = true;                                                    // :534
    for (int sidx = 0; sidx < 2; sidx++)
      if (strand_has_mods[sidx]) P.push_row(r.tid, sidx + 1, r.pos, rs[sidx].data(), (int)dest_end, c.trim5, c.trim3);   // :537-541
  }
  return EPI_OK;
}

int pack_pe(const PackCtx &c, const Rec *recs, size_t r_lo, size_t r_hi, Packed &P) {
  const uint16_t skip_flags_pe = c.skip_flags | 8;
  const uint8_t q0 = (uint8_t)(c.min_baseq - (c.min_baseq > 0 ? 1 : 0));   // src/rcpp_read_bam.cpp:30,57
  std::vector<uint8_t> tq(8192, q0), ts(8192, 0xFB), pb;
  const char *tname = nullptr;
  int t_rname = 0, t_start = 0, t_strand = 0, t_width = 0;
  auto grow = [&](size_t w) { if (w > tq.size()) { tq.resize(w, q0); ts.resize(w, 0xFB); } };
  auto push_template = [&]() {                                                   // :61-69
    P.push_row(t_rname, t_strand, t_start, ts.data(), t_width, c.trim5, c.trim3);
    std::fill(tq.begin(), tq.begin() + t_width, q0);
    std::fill(ts.begin(), ts.begin() + t_width, (uint8_t)0xFB);
  };
  for (size_t ri = r_lo; ri < r_hi; ri++) {
    const Rec &r = recs[ri];
    if ((r.flag & skip_flags_pe) || !(r.flag & 0x2) || (int)r.mapq < c.min_mapq) continue;   // :76-78
    char xg0;
    const char *xm;
    const uint8_t *pcall;
    if (!xg_xm(c, ri, r, &xg0, &xm, &pcall)) continue;                                           // :80-82
    uint32_t width;
    EPI_TRY(use_record(c, r, xm, &width));
    if (!tname || strcmp(tname, r.qname) != 0) {                                              // :85
      if (t_strand != 0) push_template();
      tname = r.qname;
      t_rname = r.tid;
      t_start = r.pos < r.mpos ? r.pos : r.mpos;                                              // :92-93
      if (r.isize == INT32_MIN) return fail(EPI_ERR_ARG, "corrupt BAM record %s: template length", r.qname);
      t_width = r.isize < 0 ? -r.isize : r.isize;                                             // :94
      t_strand = 2 - (xg0 == 'C' ? 1 : 0);                                                    // :95
      grow((size_t)t_width);
    }
    uint32_t dest_end = 0;
    if (r.pos < t_start) return fail(EPI_ERR_ARG, "corrupt BAM record %s: starts before its template", r.qname);
    const uint32_t dest0 = (uint32_t)(r.pos - t_start);                                       // :118
    if (!pcall) packed_bytes(r, xm, pb);                                                      // (nt16 << 4) | ctx_idx per query base
    const uint8_t *pbase = pcall ? pcall : pb.data();
    EPI_TRY(apply_cigar(r, dest0, [&](uint32_t qpos, uint32_t dpos, uint32_t len) {
      grow((size_t)dpos + len);
      const uint8_t *__restrict__ ql = r.qual + qpos, *__restrict__ pq = pbase + qpos;
      uint8_t *__restrict__ tqd = tq.data() + dpos, *__restrict__ tsd = ts.data() + dpos;
      for (uint32_t j = 0; j < len; j++) {                                                    // :127 strictly higher quality wins
        const bool w = ql[j] > tqd[j];                                                        // (selects, not branches: the loop vectorises)
        tqd[j] = w ? ql[j] : tqd[j];
        tsd[j] = w ? pq[j] : tsd[j];
      }
    }, &dest_end));
    if (dest_end > 0x7FFFFFFFu) return fail(EPI_ERR_ARG, "corrupt BAM record %s: template too wide", r.qname);
    if (t_width < (int)dest_end) t_width = (int)dest_end;                                     // :151
    grow((size_t)t_width);                                                                    // (a CIGAR ending in D / N)
  }
  if (t_strand != 0) push_template();                                                         // :155 (preprocess_impl has the "none")
  return EPI_OK;
}

int pack_se(const PackCtx &c, const Rec *recs, size_t r_lo, size_t r_hi, Packed &P) {
  const int min_baseq = c.min_baseq;
  std::vector<uint8_t> buf, pb;
  for (size_t ri = r_lo; ri < r_hi; ri++) {
    const Rec &r = recs[ri];
    if ((r.flag & c.skip_flags) || (int)r.mapq < c.min_mapq) continue;                        // :240-241
    char xg0;
    const char *xm;
    const uint8_t *pcall;
    if (!xg_xm(c, ri, r, &xg0, &xm, &pcall)) continue;
    uint32_t width;                                                                           // bam_cigar2rlen, :255
    EPI_TRY(use_record(c, r, xm, &width));
    buf.assign(width, 0xFB);                                                                  // :265
    uint32_t dest_end = 0;
    if (!pcall) packed_bytes(r, xm, pb);
    const uint8_t *pbase = pcall ? pcall : pb.data();
    EPI_TRY(apply_cigar(r, 0, [&](uint32_t qpos, uint32_t dpos, uint32_t len) {
      const uint8_t *__restrict__ ql = r.qual + qpos, *__restrict__ pq = pbase + qpos;
      uint8_t *__restrict__ bd = buf.data() + dpos;
      for (uint32_t j = 0; j < len; j++) bd[j] = (int)ql[j] >= min_baseq ? pq[j] : bd[j];   // :278
    }, &dest_end));
    P.push_row(r.tid, xg0 == 'C' ? 1 : 2, r.pos, buf.data(), (int)dest_end, c.trim5, c.trim3);   // :303-306
  }
  return EPI_OK;
}

// The output buffer pinned ahead (PinAhead, bam_device.hpp) is sized by an estimate (a base is at least 2.5 bytes of
// record: half a byte of SEQ, QUAL, XM): template bytes per inflated byte, sampled from the file's first records (sum of
// l_seq over sum of record sizes: a PE150 Bismark / DRAGEN file gives ~0.35, where the worst-case bound is 0.4); 0.5 when
// the sample cannot be read
double pin_ratio_sample(const BamWindows &win) {
  std::vector<Block> head;
  size_t up = 0;
  for (size_t i = 0; i < win.blocks.size() && head.size() < 4; i++) { Block b = win.blocks[i]; b.upos = up; up += b.ulen; head.push_back(b); }
  std::vector<uint8_t> buf(up + 8);
  if (up < 16 || bgzf_inflate_range(win.file.p, head, 0, head.size(), buf.data(), 1) != EPI_OK || memcmp(buf.data(), "BAM\1", 4) != 0) return 0.5;
  size_t p = 8 + (size_t)rd32(buf.data() + 4);
  uint64_t nref = p + 4 <= up ? rd32(buf.data() + p) : 0;
  p += 4;
  while (nref > 0 && p + 4 <= up) { p += 8 + (size_t)rd32(buf.data() + p); nref--; }
  uint64_t bytes = 0, bases = 0;
  while (nref == 0 && p + 36 <= up) {
    const size_t bs = rd32(buf.data() + p);
    if (bs < 32 || p + 4 + bs > up) break;
    bytes += 4 + bs; bases += rd32(buf.data() + p + 4 + 16);
    p += 4 + bs;
  }
  return bytes >= 4096 && bases > 0 && bases < bytes ? (double)bases / (double)bytes : 0.5;
}

// the buffer pinned ahead: the file's inflated size times the sampled ratio plus 15 % (files below 8 MiB: none)
void pin_ahead(const BamWindows &win, PinAhead &pin) {
  const size_t total = win.inflated_size();
  if (total < ((size_t)8 << 20)) return;
  pin_ahead_start(pin, ((size_t)((double)total * pin_ratio_sample(win) * 1.15) + ((size_t)1 << 20) + 15) / 16 * 16);
}

// mates = "anywhere": a kept record of paired-end input, wherever its mate is.  Its QNAME is kept once per template (in
// the job's qmap); its CIGAR ops, packed query bytes and qualities go to the device arena at aoff, 4 * n_cig + 2 * l_seq
// bytes rounded up to 4.
struct Kept {
  uint32_t gid;                  // template id: the order of the templates' first kept records in the file
  int32_t tid, pos, mpos, isize;
  uint32_t rspan;                // reference length of the CIGAR (M D N = X), as apply_cigar sums it
  int64_t aoff;
  int32_t n_cig, l_seq;
  uint8_t cls, strand;           // flag & 0xC0 (merge order); XG's first letter
};
inline size_t kept_bytes(const Kept &k) { return ((size_t)k.n_cig * 4 + 2 * (size_t)k.l_seq + 3) & ~(size_t)3; }

// One call of preprocessBam: what its steps below share.
//
// genome != NULL (epi_preprocess_bam_genome): the records callMethylation would call are called on the GPU, window by
// window, into packed template bytes, and the packers read them in place of XG / XM -- the result is that of
// preprocessBam(callMethylation(path)) without the BAM in between.
//
// anyorder (epi_preprocess_bam_anyorder, mates = "anywhere"): paired-end records are paired through their QNAMEs wherever
// they lie in the file.  Per window, the kept records get their template ids and their CIGAR ops, packed query bytes and
// qualities go to a device arena; at the end of the file the host orders each template's records and lays out the rows,
// and assemble_templates.hip merges them on the GPU.
struct BamJob {
  epi_bam_options opt;
  epi_templates *out = nullptr;
  epi_engine *eng = nullptr;
  epi_genome *genome = nullptr;
  bool anyorder = false;
  size_t KT = 1;                                             // threads of the host loops
  BamWindows win;
  PinAhead pin;
  PackCtx ctx;
  // check_bam's findings
  bool paired = false, tMM = false;
  bool asm_mode = false;                                     // anyorder && paired-end short-read input
  StrandTag tag = TAG_XG;                                    // with a genome: the strand tag of the records to call
  // with a genome: the window's records to call
  CallSet CS;
  int64_t ncalled = 0;
  DeviceStatePtr dev = device_state_new();                   // the GPU's buffers of the windows to call, and the arena below
  // the templates, in file order
  Packed P;                                                  // the small columns of all templates (the bytes stay in `segs`)
  std::deque<Packed> segs;                                   // what the packing threads produced, kept until the ordered copy
  std::vector<const uint8_t *> src;                          // per template: its bytes inside a segment ...
  std::vector<int32_t> len;                                  // ... and how many
  size_t nrecs_total = 0;
  // mates = "anywhere"
  QnameMap qmap;
  std::vector<Kept> kept;
  std::vector<uint8_t> wk_keep;                              // per record of the window
  std::vector<char> wk_xg;
  std::vector<const char *> wk_xm;
  std::vector<uint32_t> wk_span, wk_ri;
  std::vector<uint64_t> wk_hash;
  size_t arena_used = 0;                                     // of the device arena (dev), which is sized by the file's inflated
  int stage_k = 0;                                           // bytes: a kept record's inputs are smaller than the record
  std::vector<AsmRec> arec;                                  // kept records in merge order, template after template
  std::vector<int64_t> tpl_lo;                               // per template: its first record in arec (n + 1 entries)
  // the output
  std::vector<uint32_t> order;                               // output row -> template
  int64_t nbytes = 0;                                        // of all rows
  // EPIHIP_BAM_TIMING
  bool timing = false;
  double tm0 = 0, t_call = 0, t_pair = 0, t_upload = 0, t_group = 0;
  void lap(const char *what) { if (timing) { const double t = tnow(); fprintf(stderr, "[bam] %-10s %.3f s\n", what, t - tm0); tm0 = t; } }
};

// which of the window's records callMethylation would call, with its per-record checks
int select_calls(BamJob &J) {
  const double t0 = tnow();
  EPI_TRY(call_select(J.win.recs.begin(), J.win.recs.size(), J.tag, J.win.names, J.win.lens, J.KT, "epi_preprocess_bam", J.CS));
  J.t_call += tnow() - t0;
  return EPI_OK;
}

// The first window (at least 1024 records, or the whole file): endness, the kind of methylation tags, and whether the
// templates are assembled on the GPU.
int check_bam(BamJob &J) {
  const RecBuf &recs = J.win.recs;
  // with a genome, callMethylation's own checks come first: the strand tag, the header against the genome
  if (J.genome) {
    EPI_TRY(call_choose_tag(recs.begin(), recs.size(), nullptr, &J.tag));
    EPI_TRY(call_check_genome(J.genome, J.win.names, J.win.lens));
    EPI_TRY(select_calls(J));                                // (and its per-record checks over the whole window, before anything of it is packed)
  }
  // ---- .checkBam over the first 1024 records (src/rcpp_check_bam.cpp:40-50, R/internal.R:82-120) ----
  // (with a genome, as callMethylation's output would show them: a record to call carries XG and XM)
  size_t nrecs = 0, npaired = 0, ntempls = 0;
  bool tXG = false, tXM = false, tYD = false, tZS = false;
  const char *prevq = nullptr;
  for (const Rec &r : recs) {
    if (nrecs >= 1024) break;
    nrecs++;
    if (r.flag & 0x2) npaired++;
    const bool called = J.genome && J.CS.call[nrecs - 1];
    tXG |= called || has_tag(r, 'X', 'G'); tXM |= called || has_tag(r, 'X', 'M');
    tYD |= has_tag(r, 'Y', 'D'); tZS |= has_tag(r, 'Z', 'S');
    J.tMM |= has_tag(r, 'M', 'M') || has_tag(r, 'M', 'm');
    if (prevq && strcmp(prevq, r.qname) == 0) ntempls++;
    prevq = r.qname;
  }
  J.paired = npaired * 2 > nrecs;
  const bool sorted = ntempls > 0 && (ntempls >= nrecs / 2 || ntempls >= npaired / 2);
  if (nrecs == 0) return fail(EPI_ERR_ARG, "Empty file provided! Exiting");
  if (!tXG && tYD) return fail(EPI_ERR_ARG, "No XG tags found (though YD tags are there)! BWA-meth alignment? If so, make methylation calls using epialleleR::callMethylation. Exiting");
  if (!tXG && tZS) return fail(EPI_ERR_ARG, "No XG tags found (though ZS tags are there)! BSMAP alignment? If so, make methylation calls using epialleleR::callMethylation. Exiting");
  if (!tXM && tXG) return fail(EPI_ERR_ARG, "No XM tags found! Was methylation called successfully? If not, make methylation calls using epialleleR::callMethylation. Exiting");
  if (!J.tMM && !(tXG && tXM)) return fail(EPI_ERR_ARG, "No known methylation tags found! Exiting");
  if (J.paired && !sorted && !J.anyorder) return fail(EPI_ERR_ARG, "BAM file seems to be paired-end but not sorted by name! Please sort using 'samtools sort -n -o out.bam in.bam'. Exiting");
  if (J.opt.paired >= 0 && (J.opt.paired != 0) != J.paired) return fail(EPI_ERR_ARG, "Expected endness is different from detected! Exiting");
  J.asm_mode = J.anyorder && J.paired && !J.tMM;
  if (J.asm_mode) EPI_TRY(arena_reserve(J.dev.get(), J.eng, J.win.inflated_size()));
  return EPI_OK;
}

// with a genome: records [0, r_end), the ones about to be packed, are called on the GPU -- once, here
int call_window(BamJob &J, size_t r_end) {
  const double t0 = tnow();
  CallSet &CS = J.CS;
  EPI_TRY(call_pack_inputs(J.win.recs.begin(), r_end, J.KT, "epi_preprocess_bam", CS));
  const int64_t ncall = (int64_t)CS.crec.size();
  J.ncalled += ncall;
  if (!J.tMM)                                                // (the MM/ML packer reads no XG / XM)
    EPI_TRY(device_call_window(J.dev.get(), J.eng, J.genome, CS.crec.data(), ncall, CS.cigar.data(), CS.ncig, CS.seq.data(),
                               CS.nseq, CS.nxm, CALL_PACKED, CS.xm.data()));
  J.t_call += tnow() - t0;
  return EPI_OK;
}

// packs records [0, r_end) of the current window with the job's threads and appends the templates to P
int pack_window(BamJob &J, size_t r_end) {
  const RecBuf &recs = J.win.recs;
  std::vector<size_t> cut = even_cuts(r_end, r_end < 1024 ? 1 : J.KT);
  if (!J.tMM && J.paired)                                    // a template's records are neighbours with one QNAME
    for (size_t &c : cut)
      while (c > 0 && c < r_end && strcmp(recs[c].qname, recs[c - 1].qname) == 0) c++;
  std::vector<Packed> part(cut.size() - 1);
  EPI_TRY(fan_out(cut, "epi_preprocess_bam", "packing templates", [&](size_t k, size_t lo, size_t hi) -> int {
    Packed &q = part[k];
    q.off.push_back(0);
    size_t bases = 0;                                        // (one allocation instead of a doubling series per column)
    for (size_t i = lo; i < hi; i++) bases += (size_t)recs[i].l_seq;
    q.bytes.reserve(bases + bases / 8 + 4096);
    q.off.reserve(hi - lo + 2); q.rname.reserve(hi - lo + 1); q.strand.reserve(hi - lo + 1); q.start.reserve(hi - lo + 1);
    return J.tMM ? pack_mm(J.ctx, recs.begin(), lo, hi, q) : J.paired ? pack_pe(J.ctx, recs.begin(), lo, hi, q) : pack_se(J.ctx, recs.begin(), lo, hi, q);
  }));
  // the packed bytes stay where the threads wrote them (a segment per thread and window): only the small columns are
  // concatenated, and the final ordered copy reads the segments directly
  Packed &P = J.P;
  for (Packed &p : part) {
    J.segs.push_back(std::move(p));
    const Packed &q = J.segs.back();
    P.rname.insert(P.rname.end(), q.rname.begin(), q.rname.end());
    P.strand.insert(P.strand.end(), q.strand.begin(), q.strand.end());
    P.start.insert(P.start.end(), q.start.begin(), q.start.end());
    for (size_t i = 0; i + 1 < q.off.size(); i++) {
      J.src.push_back(q.bytes.data() + q.off[i]);
      J.len.push_back((int32_t)(q.off[i + 1] - q.off[i]));
    }
  }
  return EPI_OK;
}

// mates = "anywhere": the inputs of kept records [k0, kept.size()), all of this window, go to the device arena through
// the engine's two pinned staging buffers: filled by the threads while the copy stream drains the other one
int upload_kept(BamJob &J, size_t k0, size_t wbytes) {
  const RecBuf &recs = J.win.recs;
  const std::vector<Kept> &kept = J.kept;
  if (J.arena_used + wbytes > arena_capacity(J.dev.get())) return fail(EPI_ERR_STATE, "epi_preprocess_bam_anyorder: device arena too small");
  auto fill = [&](size_t i, uint8_t *o) {                   // kept record k0 + i -> its arena bytes at o
    const Rec &r = recs[J.wk_ri[i]];
    if (r.n_cigar) memcpy(o, r.cigar, 4 * (size_t)r.n_cigar);
    o += 4 * (size_t)r.n_cigar;
    pack_query(r, J.wk_xm[J.wk_ri[i]], o);
    if (r.l_seq) memcpy(o + r.l_seq, r.qual, (size_t)r.l_seq);
  };
  const size_t nk = kept.size() - k0;
  for (size_t i = 0; i < nk;) {
    uint8_t *st;
    size_t cap;
    EPI_TRY(arena_stage(J.eng, J.stage_k, &st, &cap));
    size_t j = i, bytes = 0;
    while (j < nk && bytes + kept_bytes(kept[k0 + j]) <= cap) bytes += kept_bytes(kept[k0 + j++]);
    if (j == i) {                                           // one record larger than a staging buffer: a copy of its own
      std::vector<uint8_t> big(kept_bytes(kept[k0 + i]));
      fill(i, big.data());
      EPI_TRY(arena_write(J.dev.get(), kept[k0 + i].aoff, big.data(), big.size()));
      i++;
      continue;
    }
    const int64_t a0 = kept[k0 + i].aoff;
    EPI_TRY(parallel_ranges(J.KT, j - i, "epi_preprocess_bam", [&](size_t lo, size_t hi) -> int {
      for (size_t x = i + lo; x < i + hi; x++) fill(x, st + (kept[k0 + x].aoff - a0));
      return EPI_OK;
    }));
    EPI_TRY(arena_send(J.dev.get(), J.eng, J.stage_k, a0, bytes));
    J.stage_k ^= 1;
    i = j;
  }
  return EPI_OK;
}

// mates = "anywhere": the window's records [0, nrec): which are kept (pack_pe's filters and checks), their template ids,
// and their inputs queued for upload
int collect_window(BamJob &J, size_t nrec) {
  const double t0 = tnow();
  const RecBuf &recs = J.win.recs;
  const PackCtx &c = J.ctx;
  const uint16_t skip_flags_pe = c.skip_flags | 8;
  J.wk_keep.resize(nrec); J.wk_xg.resize(nrec); J.wk_xm.resize(nrec); J.wk_span.resize(nrec); J.wk_hash.resize(nrec);
  EPI_TRY(parallel_ranges(J.KT, nrec, "epi_preprocess_bam", [&](size_t lo, size_t hi) -> int {
    for (size_t ri = lo; ri < hi; ri++) {
      const Rec &r = recs[ri];
      J.wk_keep[ri] = 0;
      if ((r.flag & skip_flags_pe) || !(r.flag & 0x2) || (int)r.mapq < c.min_mapq) continue;   // pack_pe's filters
      char xg0;
      const char *xm;
      const uint8_t *pcall;
      if (!xg_xm(c, ri, r, &xg0, &xm, &pcall)) continue;
      uint32_t width, span = 0;
      EPI_TRY(use_record(c, r, xm, &width));
      EPI_TRY(apply_cigar(r, 0, [](uint32_t, uint32_t, uint32_t) {}, &span));
      J.wk_keep[ri] = 1; J.wk_xg[ri] = xg0; J.wk_xm[ri] = xm; J.wk_span[ri] = span;
      J.wk_hash[ri] = QnameMap::hash(r.qname);
    }
    return EPI_OK;
  }));
  const size_t k0 = J.kept.size();                           // ids in file order: the same for every nthreads
  J.wk_ri.clear();
  size_t wbytes = 0;
  for (size_t ri = 0; ri < nrec; ri++) {
    if (!J.wk_keep[ri]) continue;
    const Rec &r = recs[ri];
    Kept k;
    k.gid = J.qmap.find_or_add(r.qname, J.wk_hash[ri]);
    k.tid = r.tid; k.pos = r.pos; k.mpos = r.mpos; k.isize = r.isize; k.rspan = J.wk_span[ri];
    k.n_cig = (int32_t)r.n_cigar; k.l_seq = r.l_seq;
    k.cls = (uint8_t)(r.flag & 0xC0); k.strand = (uint8_t)(2 - (J.wk_xg[ri] == 'C' ? 1 : 0));
    k.aoff = (int64_t)(J.arena_used + wbytes);
    wbytes += kept_bytes(k);
    J.kept.push_back(k);
    J.wk_ri.push_back((uint32_t)ri);
  }
  const double t1 = tnow();
  J.t_pair += t1 - t0;
  EPI_TRY(upload_kept(J, k0, wbytes));
  J.arena_used += wbytes;
  J.t_upload += tnow() - t1;
  return EPI_OK;
}

// mates = "anywhere": every template's records are known now.  Each one's records go in merge order (flag & 0xC0, then
// file order: READ1 before READ2), the first gives rname, start, width and strand, and the rest may widen it -- pack_pe's
// rules and errors on G(F), without touching a byte (the kernel merges them once the rows have their places).
int group_templates(BamJob &J) {
  std::vector<Kept> &kept = J.kept;
  std::vector<int64_t> &tpl_lo = J.tpl_lo;
  const size_t G = J.qmap.size(), NK = kept.size();
  tpl_lo.assign(G + 1, 0);
  for (const Kept &k : kept) tpl_lo[k.gid + 1]++;
  for (size_t g = 0; g < G; g++) tpl_lo[g + 1] += tpl_lo[g];
  std::vector<uint32_t> mo(NK);                             // kept records by template, in file order (a stable counting sort)
  {
    std::vector<int64_t> cur(tpl_lo.begin(), tpl_lo.end() - 1);
    for (size_t i = 0; i < NK; i++) mo[(size_t)cur[kept[i].gid]++] = (uint32_t)i;
  }
  J.arec.resize(NK);
  J.P.rname.reserve(G); J.P.strand.reserve(G); J.P.start.reserve(G); J.len.reserve(G);
  for (size_t g = 0; g < G; g++) {
    uint32_t *m = mo.data() + tpl_lo[g], nm = (uint32_t)(tpl_lo[g + 1] - tpl_lo[g]);
    for (uint32_t a = 1; a < nm; a++)                       // (stable insertion sort by flag & 0xC0: a template has few records)
      for (uint32_t b = a; b > 0 && kept[m[b]].cls < kept[m[b - 1]].cls; b--) std::swap(m[b], m[b - 1]);
    const Kept &f = kept[m[0]];
    const int t_start = f.pos < f.mpos ? f.pos : f.mpos;                                     // :92-93
    if (f.isize == INT32_MIN) return fail(EPI_ERR_ARG, "corrupt BAM record %s: template length", J.qmap.name((uint32_t)g));
    int t_width = f.isize < 0 ? -f.isize : f.isize;                                          // :94
    for (uint32_t a = 0; a < nm; a++) {
      const Kept &k = kept[m[a]];
      if (k.pos < t_start) return fail(EPI_ERR_ARG, "corrupt BAM record %s: starts before its template", J.qmap.name((uint32_t)g));
      const uint32_t dest0 = (uint32_t)(k.pos - t_start), dest_end = dest0 + k.rspan;     // :118 (apply_cigar's sum)
      if (dest_end > 0x7FFFFFFFu) return fail(EPI_ERR_ARG, "corrupt BAM record %s: template too wide", J.qmap.name((uint32_t)g));
      if (t_width < (int)dest_end) t_width = (int)dest_end;                                  // :151
      AsmRec &x = J.arec[(size_t)tpl_lo[g] + a];
      x.arena_off = k.aoff; x.dest0 = (int32_t)dest0; x.n_cig = k.n_cig; x.l_seq = k.l_seq; x.pad = 0;
    }
    J.P.rname.push_back(f.tid + 1);                                                          // :61-69
    J.P.strand.push_back(f.strand);
    J.P.start.push_back(t_start + J.ctx.trim5 + 1);
    const int keep = t_width - (J.ctx.trim5 + J.ctx.trim3);
    J.len.push_back(keep > 0 ? keep : 0);
  }
  std::vector<Kept>().swap(kept);
  return EPI_OK;
}

// ---- templid := 0..N-1 ; setorder(rname, start) -- stable (R/internal.R:193-195) ----
int sort_templates(BamJob &J) {
  const Packed &P = J.P;
  const size_t n = P.rname.size();
  std::vector<uint32_t> &order = J.order;
  order.resize(n);
  std::iota(order.begin(), order.end(), 0u);
  auto less = [&](uint32_t a, uint32_t b) {
    if (P.rname[a] != P.rname[b]) return P.rname[a] < P.rname[b];
    return P.start[a] < P.start[b];
  };
  // stable: ranges sorted by the threads, then merged pairwise (std::inplace_merge keeps equal keys in order)
  size_t K = 1;
  while (K * 2 <= J.KT && n / (K * 2) >= 65536) K *= 2;
  const std::vector<size_t> cut = even_cuts(n, K);
  EPI_TRY(fan_out(cut, "epi_preprocess_bam", "sorting templates", [&](size_t, size_t lo, size_t hi) -> int {
    std::stable_sort(order.begin() + lo, order.begin() + hi, less);
    return EPI_OK;
  }));
  for (size_t w = 1; w < K; w *= 2) {                        // merge runs of w ranges
    std::vector<std::thread> th;
    for (size_t k = 0; k + w < K; k += 2 * w) {
      const size_t lo = cut[k], mid = cut[k + w], hi = cut[k + 2 * w < K ? k + 2 * w : K];
      th.emplace_back([&, lo, mid, hi]() { std::inplace_merge(order.begin() + lo, order.begin() + mid, order.begin() + hi, less); });
    }
    for (auto &t : th) t.join();
  }
  return EPI_OK;
}

// the output columns: the bytes in the buffer pinned ahead where it fits, and every row's offset
int allocate_output(BamJob &J) {
  epi_templates *out = J.out;
  const size_t n = J.order.size();
  size_t nbytes = 0;
  for (size_t i = 0; i < n; i++) nbytes += (size_t)J.len[i];
  size_t cap = (nbytes + 15) / 16 * 16 + 64;
  void *xmp = nullptr;
  PinAhead &pin = J.pin;
  pin.wait();
  // the buffer pinned while the file was being read -- unless it turned out too small, or more than a quarter larger
  // than needed (page-locked memory stays pinned for the life of the templates: then the exact size is allocated)
  if (pin.ok && pin.cap >= cap && pin.cap <= cap + cap / 4 + ((size_t)4 << 20)) {
    xmp = pin.p; out->pinned = 1;
    pin.p = nullptr; pin.ok = false;
  } else {
    pin.release();
    if (pinned_alloc(cap, &xmp)) out->pinned = 1;
    else { xmp = malloc(cap); out->pinned = 0; }
  }
  out->xm = (uint8_t *)xmp;
  out->off = (int64_t *)malloc((n + 1) * sizeof(int64_t));
  out->rname = (int32_t *)malloc((n + 1) * sizeof(int32_t));
  out->strand = (int32_t *)malloc((n + 1) * sizeof(int32_t));
  out->start = (int32_t *)malloc((n + 1) * sizeof(int32_t));
  out->target_names = (char **)calloc(J.win.names.size() + 1, sizeof(char *));
  if (!out->xm || !out->off || !out->rname || !out->strand || !out->start || !out->target_names) {
    epi_templates_free(out);
    return fail(EPI_ERR_NOMEM, "epi_preprocess_bam: out of host memory");
  }
  int64_t w = 0;
  for (size_t i = 0; i < n; i++) { out->off[i] = w; w += J.len[J.order[i]]; }
  out->off[n] = w;
  J.nbytes = w;
  return EPI_OK;
}

// the ordered copy, by ranges of output rows (mates = "anywhere": the small columns only, the GPU writes the bytes)
int copy_ordered(BamJob &J) {
  epi_templates *out = J.out;
  const size_t n = J.order.size();
  return fan_out(even_cuts(n, n < 4096 ? 1 : J.KT), "epi_preprocess_bam", "copying templates", [&](size_t, size_t lo, size_t hi) -> int {
    for (size_t i = lo; i < hi; i++) {
      const uint32_t t = J.order[i];
      if (J.len[t] && !J.asm_mode) memcpy(out->xm + out->off[i], J.src[t], (size_t)J.len[t]);
      out->rname[i] = J.P.rname[t]; out->strand[i] = J.P.strand[t]; out->start[i] = J.P.start[t];
    }
    return EPI_OK;
  });
}

// mates = "anywhere": the rows, merged on the GPU in their output slots
int assemble_on_gpu(BamJob &J) {
  const size_t n = J.order.size();
  std::vector<AsmTpl> tpl(n);
  int64_t qbytes = 0;
  for (size_t i = 0; i < n; i++) {
    const uint32_t t = J.order[i];
    AsmTpl &x = tpl[i];
    x.out_off = J.out->off[i]; x.rec_lo = J.tpl_lo[t]; x.nrec = (int32_t)(J.tpl_lo[t + 1] - J.tpl_lo[t]); x.keep = J.len[t];
    x.q_off = 0;
    if (J.len[t] > kAsmLdsWidth) { x.q_off = qbytes; qbytes += J.len[t]; }
  }
  const uint8_t q0 = (uint8_t)(J.ctx.min_baseq - (J.ctx.min_baseq > 0 ? 1 : 0));   // src/rcpp_read_bam.cpp:30,57
  double t_sync = 0, t_kernel = 0, t_d2h = 0;
  EPI_TRY(arena_assemble(J.dev.get(), J.eng, tpl.data(), (int64_t)n, J.arec.data(), (int64_t)J.arec.size(), q0, J.ctx.trim5,
                         J.nbytes, qbytes, J.out->xm, &t_sync, &t_kernel, &t_d2h));
  J.t_upload += t_sync;
  if (J.timing)
    fprintf(stderr, "[bam] (anywhere: inflate %.3f s, parse %.3f s, pairing %.3f s, upload %.3f s, grouping %.3f s, "
                    "kernel %.3f s, D2H %.3f s)\n", J.win.t_inflate, J.win.t_parse, J.t_pair, J.t_upload, J.t_group, t_kernel, t_d2h);
  return EPI_OK;
}

void finish(BamJob &J, int64_t *ncalled_out) {
  epi_templates *out = J.out;
  const std::vector<std::string> &names = J.win.names;
  // 0xFB padding up to the 16-byte boundary the kernels may read to, plus a little (a buffer pinned ahead can be much
  // larger than the templates: its tail stays untouched and is not part of xm_capacity)
  const size_t padded = ((size_t)J.nbytes + 15) / 16 * 16 + 64;
  memset(out->xm + J.nbytes, 0xFB, padded - (size_t)J.nbytes);
  J.lap("sort+copy");
  out->n = (int64_t)J.order.size();
  out->nbytes = J.nbytes;
  out->xm_capacity = (int64_t)padded;
  out->nrecs = (int64_t)J.nrecs_total;
  if (ncalled_out) *ncalled_out = J.ncalled;
  out->paired = J.paired ? 1 : 0;
  out->n_targets = (int32_t)names.size();
  for (size_t i = 0; i < names.size(); i++) out->target_names[i] = strdup(names[i].c_str());
}

// option defaults, the thread cap and what the packers read of them
int set_options(BamJob &J, const epi_bam_options *opt_in) {
  epi_bam_options &opt = J.opt;
  if (opt_in) opt = *opt_in;
  else { memset(&opt, 0, sizeof(opt)); opt.skip_secondary = opt.skip_qcfail = opt.skip_supplementary = 1; opt.paired = -1; opt.nthreads = 1; opt.min_prob = -1; opt.highest_prob = 1; }
  if (opt.trim5 < 0 || opt.trim3 < 0) return fail(EPI_ERR_ARG, "trim must be non-negative");
  J.KT = thread_cap(opt.nthreads);
  uint16_t skip_flags = 4;
  if (opt.skip_secondary) skip_flags |= 256;
  if (opt.skip_qcfail) skip_flags |= 512;
  if (opt.skip_duplicates) skip_flags |= 1024;
  if (opt.skip_supplementary) skip_flags |= 2048;
  J.ctx = PackCtx{skip_flags, opt.min_mapq, opt.min_baseq, opt.min_prob, opt.highest_prob, opt.trim5, opt.trim3, 0, nullptr};
  J.timing = epi::options().bam_timing != 0;
  J.tm0 = tnow();
  return EPI_OK;
}

int preprocess_impl(const char *path, const epi_bam_options *opt_in, epi_templates *out, epi_engine *eng,
                    epi_genome *genome, int64_t *ncalled_out, bool anyorder) {
  BamJob J;
  J.out = out; J.eng = eng; J.genome = genome; J.anyorder = anyorder;
  EPI_TRY(set_options(J, opt_in));
  BamWindows &win = J.win;
  // with a genome, the header messages are callMethylation's: it reads the file first
  EPI_TRY(win.open(path, J.opt.window_kib, (size_t)256 << 20, J.opt.nthreads, genome ? "Unable to read input BAM header" : "Unable to read BAM header"));
  pin_ahead(win, J.pin);
  bool checked = false;
  for (;;) {
    bool final;
    EPI_TRY(win.next(&final));
    if (!checked) {
      if (win.recs.size() < 1024 && !final) { win.keep_all(); continue; }   // .checkBam looks at the first 1024 records
      J.lap("index");
      J.ctx.n_ref = win.names.size();
      J.ctx.calls = genome ? &J.CS : nullptr;
      EPI_TRY(check_bam(J));
      checked = true;
    } else if (genome) {
      EPI_TRY(select_calls(J));
    }
    // paired-end: the records of the window's last QNAME wait for the next window (their mate may be in it)
    size_t r_end = win.recs.size();
    if (!final && J.paired && !J.tMM && !J.asm_mode && r_end > 0) {
      const char *lastq = win.recs[r_end - 1].qname;
      while (r_end > 0 && strcmp(win.recs[r_end - 1].qname, lastq) == 0) r_end--;
      if (r_end == 0) { win.keep_all(); continue; }          // one template fills the window: read on
    }
    if (genome) EPI_TRY(call_window(J, r_end));
    if (J.asm_mode) EPI_TRY(collect_window(J, r_end));
    else EPI_TRY(pack_window(J, r_end));
    J.nrecs_total += r_end;
    win.consume(r_end);
    if (final) break;
  }
  const double t_g0 = tnow();
  if (J.asm_mode) EPI_TRY(group_templates(J));
  if (!J.tMM && J.paired && J.P.rname.empty()) {             // the reference pushes its (never opened) template all the same, :155
    J.P.rname.push_back(1); J.P.strand.push_back(0); J.P.start.push_back(J.ctx.trim5 + 1); J.src.push_back(nullptr); J.len.push_back(0);
    if (J.asm_mode) J.tpl_lo.push_back(J.tpl_lo.back());
  }
  win.release();
  J.t_group = tnow() - t_g0;
  J.lap("pack");
  if (J.timing && genome) fprintf(stderr, "[bam] (of which call selection, inputs and GPU %.3f s)\n", J.t_call);
  EPI_TRY(sort_templates(J));
  EPI_TRY(allocate_output(J));
  EPI_TRY(copy_ordered(J));
  if (J.asm_mode) EPI_TRY(assemble_on_gpu(J));
  finish(J, ncalled_out);
  return EPI_OK;
}

// the three preprocessBam entry points: nothing may unwind through the C boundary, and a failed call leaves *out empty
int preprocess_entry(const char *path, const epi_bam_options *opt_in, epi_templates *out, epi_engine *eng, epi_genome *genome,
                     int64_t *ncalled, bool anyorder) {
  int rc;
  try {
    rc = preprocess_impl(path, opt_in, out, eng, genome, ncalled, anyorder);
  } catch (const std::bad_alloc &) {
    rc = fail(EPI_ERR_NOMEM, "epi_preprocess_bam: out of host memory");
  } catch (...) {
    rc = fail(EPI_ERR_ARG, "epi_preprocess_bam: unexpected failure while reading %s", path);
  }
  if (rc != EPI_OK) { epi_templates_free(out); if (ncalled) *ncalled = 0; }
  return rc;
}

}  // namespace

extern "C" {

void epi_templates_free(epi_templates *t) {
  if (!t) return;
  if (t->xm) { if (t->pinned) pinned_free(t->xm); else free(t->xm); }
  free(t->off); free(t->rname); free(t->strand); free(t->start);
  if (t->target_names) { for (int32_t i = 0; i < t->n_targets; i++) free(t->target_names[i]); free(t->target_names); }
  memset(t, 0, sizeof(*t));
}

int epi_preprocess_bam(const char *path, const epi_bam_options *opt_in, epi_templates *out) {
  if (!path || !out) return fail(EPI_ERR_ARG, "epi_preprocess_bam: NULL argument");
  memset(out, 0, sizeof(*out));
  return preprocess_entry(path, opt_in, out, nullptr, nullptr, nullptr, false);
}

int epi_preprocess_bam_genome(epi_engine *eng, const char *path, const epi_bam_options *opt_in, epi_genome *g,
                              epi_templates *out, int64_t *ncalled) {
  if (!path || !out || !g || !ncalled) return fail(EPI_ERR_ARG, "epi_preprocess_bam_genome: NULL argument");
  memset(out, 0, sizeof(*out));
  *ncalled = 0;
  EPI_TRY(device_engine(&eng, "epi_preprocess_bam_genome: the calls are made on the GPU"));   // no device: fails here, before the file is read
  return preprocess_entry(path, opt_in, out, eng, g, ncalled, false);
}

int epi_preprocess_bam_anyorder(epi_engine *eng, const char *path, const epi_bam_options *opt_in, epi_templates *out) {
  if (!path || !out) return fail(EPI_ERR_ARG, "epi_preprocess_bam_anyorder: NULL argument");
  memset(out, 0, sizeof(*out));
  EPI_TRY(device_engine(&eng, "epi_preprocess_bam_anyorder: templates are assembled on the GPU"));   // (as above)
  return preprocess_entry(path, opt_in, out, eng, nullptr, nullptr, true);
}

}  // extern "C"
