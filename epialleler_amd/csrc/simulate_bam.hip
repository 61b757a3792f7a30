// simulateBam's record assembly (src/rcpp_simulate_bam.cpp restated: HTSlib's sam_parse_cigar, bam_set1, bam_write1 and
// bam_aux_update_*) on the GPU.  The host ships only the columns the caller supplied, at their own lengths; record i
// reads element (i % period) % len of each (include/epihip.h, epi_sim_column).  The defaults that depend on the record
// (qname "q%04d", the random bases, the "<l>M" CIGAR, the 'F' qualities, tlen = l_seq) are made here, not shipped.
//
//   k_sim_size   one thread per record: the CIGAR string parsed, the record's encoded size (SAM spec 4.2, tags
//                included) and its error code; the first failing record by atomicMin.  Every record is checked before
//                the output file is opened.
//   (scan)       util.hip's exclusive u32 scan of the sizes of one window: the records' offsets in it.
//   k_sim_write  one wavefront per record, four per workgroup: the lanes stride over each region of the record (fixed
//                fields, qname, CIGAR ops, nt16 nibbles, qualities, tags) with byte stores, so a 10 kb read is spread
//                over the wave like a short one.  The CIGAR string is short: every lane parses it (same addresses,
//                uniform work) and lane 0 stores the ops.
// The host cuts windows of ~64 MiB of output, copies each to one of two pinned buffers and hands it to the BGZF writer's
// threads while the next window is built.
#include <chrono>
#include <stdio.h>
#include <string.h>
#include <sys/stat.h>
#include <unistd.h>
#include <string>
#include <thread>
#include <vector>
#include "common.hpp"

namespace epi {
namespace {

constexpr int kWaves = 4;                              // records per workgroup of 256 threads (as k_call_xm)
constexpr uint64_t kSeqStream = 0x53494D;              // hash3 stream of the random bases ("SIM")
constexpr int64_t kMaxCigarLen = (1LL << 28) - 1;      // sam_parse_cigar: hts_str2uint(.., 28 bits, ..)
enum SimErr : uint8_t { ERR_NONE = 0, ERR_CIGAR = 1, ERR_RECORD = 2, ERR_QUAL = 3, ERR_QNAME = 4, ERR_NCIGAR = 5, ERR_SIZE = 6 };
enum { F_QNAME = 0, F_FLAG, F_TID, F_POS, F_MAPQ, F_CIGAR, F_MTID, F_MPOS, F_ISIZE, F_SEQ, F_QUAL };

struct SimCol {                 // device copy of an epi_sim_column
  const uint8_t *values;
  const int64_t *offsets;
  int64_t len, period;
  int32_t kind;
  uint8_t type, n0, n1, pad;
};

__device__ __forceinline__ int64_t col_elem(const SimCol &c, int64_t i) { return (i % c.period) % c.len; }
__device__ __forceinline__ int32_t col_i32(const SimCol &c, int64_t i) {
  return reinterpret_cast<const int32_t *>(c.values)[col_elem(c, i)];
}
__device__ __forceinline__ uint32_t col_u32(const SimCol &c, int64_t j) { return reinterpret_cast<const uint32_t *>(c.values)[j]; }

// bam_cigar_table: M I D N S H P = X B -> 0 .. 9, anything else -1
__device__ __forceinline__ int cigar_op(uint8_t ch) {
  switch (ch) {
    case 'M': return 0; case 'I': return 1; case 'D': return 2; case 'N': return 3; case 'S': return 4;
    case 'H': return 5; case 'P': return 6; case '=': return 7; case 'X': return 8; case 'B': return 9;
    default: return -1;
  }
}
// BAM_CIGAR_TYPE: bit 0 consumes the query, bit 1 the reference
__device__ __forceinline__ uint32_t cigar_type(int op) { return (0x3C1A7u >> (op << 1)) & 3u; }

__device__ __forceinline__ bool is_digit(uint8_t c) { return c >= '0' && c <= '9'; }

// sam_parse_cigar: "*" is no ops, a string without operator letters is no ops; otherwise one op per non-digit, each a
// run of digits (< 2^28) and an operator.  Returns the number of ops, -1 when malformed; lane 0 also stores the ops.
__device__ __forceinline__ int64_t parse_cigar(const uint8_t *s, int64_t n, int64_t *qlen, int64_t *rlen, uint8_t *out) {
  *qlen = 0; *rlen = 0;
  if (n > 0 && s[0] == '*') return 0;
  int64_t nops = 0;
  for (int64_t k = 0; k < n; k++) nops += is_digit(s[k]) ? 0 : 1;
  int64_t p = 0;
  for (int64_t o = 0; o < nops; o++) {
    int64_t len = 0, q = p;
    while (q < n && is_digit(s[q])) {
      len = len * 10 + (s[q] - '0');
      if (len > kMaxCigarLen) return -1;
      q++;
    }
    if (q == p || q >= n) return -1;
    const int op = cigar_op(s[q]);
    if (op < 0) return -1;
    const uint32_t t = cigar_type(op);
    if (t & 1u) *qlen += len;
    if (t & 2u) *rlen += len;
    if (out) {
      const uint32_t v = ((uint32_t)len << 4) | (uint32_t)op;
      out[4 * o] = (uint8_t)v; out[4 * o + 1] = (uint8_t)(v >> 8); out[4 * o + 2] = (uint8_t)(v >> 16); out[4 * o + 3] = (uint8_t)(v >> 24);
    }
    p = q + 1;
  }
  return nops;
}

// seq_nt16_table: "=ACMGRSVTWYHKDBN" either case, U as T, the digits 0-3 as 1, 2, 4, 8 (HTSlib's colour-space row),
// everything else N
__device__ __forceinline__ uint32_t nt16(uint8_t c) {
  if (c >= '0' && c <= '3') return 1u << (c - '0');
  if (c == '=') return 0;
  c &= 0xDF;
  switch (c) {
    case 'A': return 1; case 'C': return 2; case 'M': return 3; case 'G': return 4; case 'R': return 5; case 'S': return 6;
    case 'V': return 7; case 'T': case 'U': return 8; case 'W': return 9; case 'Y': return 10; case 'H': return 11;
    case 'K': return 12; case 'D': return 13; case 'B': return 14;
    default: return 15;
  }
}

__device__ __forceinline__ uint8_t random_base(uint64_t seed, int64_t j, int64_t k) {
  return (uint8_t)"ACTG"[hash3(seed, kSeqStream, ((uint64_t)j << 32) | (uint64_t)k) >> 62];
}

// bam_aux_update_int: the narrowest type that holds the value
__device__ __forceinline__ uint8_t int_tag_type(int32_t v) {
  return v < -32768 ? 'i' : v < -128 ? 's' : v < 0 ? 'c' : v <= 255 ? 'C' : v <= 65535 ? 'S' : 'I';
}
__device__ __forceinline__ int type_size(uint8_t t) { return (t == 'c' || t == 'C') ? 1 : (t == 's' || t == 'S') ? 2 : 4; }

__device__ __forceinline__ int32_t ndigits(int64_t v) { int32_t d = 1; while (v >= 10) { v /= 10; d++; } return d; }

// hts_reg2bin(beg, end, 14, 5) as bam_set1 calls it, truncated to the record's 16 bits
__device__ __forceinline__ uint32_t reg2bin(int64_t beg, int64_t end) {
  --end;
  if (beg >> 14 == end >> 14) return (uint32_t)(((1 << 15) - 1) / 7 + (beg >> 14)) & 0xFFFFu;
  if (beg >> 17 == end >> 17) return (uint32_t)(((1 << 12) - 1) / 7 + (beg >> 17)) & 0xFFFFu;
  if (beg >> 20 == end >> 20) return (uint32_t)(((1 << 9) - 1) / 7 + (beg >> 20)) & 0xFFFFu;
  if (beg >> 23 == end >> 23) return (uint32_t)(((1 << 6) - 1) / 7 + (beg >> 23)) & 0xFFFFu;
  if (beg >> 26 == end >> 26) return (uint32_t)(((1 << 3) - 1) / 7 + (beg >> 26)) & 0xFFFFu;
  return 0;
}

struct Str { const uint8_t *p; int64_t n; };
__device__ __forceinline__ Str col_str(const SimCol &c, int64_t j) {
  const int64_t a = c.offsets[j], b = c.offsets[j + 1];
  return Str{c.values + a, b - a};
}

// Everything about record i but its bytes.  Wave-uniform in k_sim_write (every lane computes the same).
struct Layout {
  Str qname, cigar, seq, qual;
  int64_t seq_j;              // element of the random seq column
  int64_t l_qname;            // without the NUL; 0 -> "*"
  int64_t qname_num;          // default qname: i + 1
  int64_t l_seq, ncig, qlen, rlen;
  int64_t tag_bytes, size;    // size: the record with its block_size field
  int32_t flag;
  uint8_t err;
};

__device__ __forceinline__ int64_t tag_size(const SimCol &c, int64_t i, int64_t *elem) {
  const int64_t j = col_elem(c, i);
  *elem = j;
  switch (c.kind) {
    case EPI_SIM_I32: return 3 + type_size(int_tag_type((int32_t)col_u32(c, j)));
    case EPI_SIM_F32: return 7;
    case EPI_SIM_STR: return 3 + (c.offsets[j + 1] - c.offsets[j]) + 1;
    default: return 8 + (c.offsets[j + 1] - c.offsets[j]) * type_size(c.type);
  }
}

__device__ __forceinline__ Layout record_layout(const SimCol *cols, int ntags, int64_t i, uint8_t *cig_out) {
  Layout L = {};
  L.err = ERR_NONE;
  const SimCol &cs = cols[F_SEQ];
  if (cs.kind == EPI_SIM_RANDOM) {
    L.seq_j = col_elem(cs, i);
    L.seq = Str{nullptr, 0};
    L.l_seq = (int64_t)(int32_t)col_u32(cs, L.seq_j);
  } else {
    L.seq_j = 0;
    L.seq = col_str(cs, col_elem(cs, i));
    L.l_seq = L.seq.n;
  }
  if (cols[F_QNAME].kind == EPI_SIM_STR) {
    L.qname = col_str(cols[F_QNAME], col_elem(cols[F_QNAME], i));
    L.l_qname = L.qname.n > 0 ? L.qname.n : 1;          // bam_set1: an empty name is "*"
    L.qname_num = 0;
  } else {
    L.qname = Str{nullptr, 0};
    L.qname_num = i + 1;
    const int32_t d = ndigits(i + 1);
    L.l_qname = 1 + (d < 4 ? 4 : d);
  }
  L.flag = col_i32(cols[F_FLAG], i);
  if (cols[F_CIGAR].kind == EPI_SIM_STR) {
    L.cigar = col_str(cols[F_CIGAR], col_elem(cols[F_CIGAR], i));
    int64_t ql, rl;
    L.ncig = parse_cigar(L.cigar.p, L.cigar.n, &ql, &rl, cig_out);
    L.qlen = ql; L.rlen = rl;
    if (L.ncig < 0) { L.err = ERR_CIGAR; L.ncig = 0; }
  } else {                                              // "<l_seq>M"
    L.cigar = Str{nullptr, 0};
    L.ncig = 1;
    L.qlen = L.rlen = L.l_seq;
    if (L.l_seq > kMaxCigarLen) { L.err = ERR_CIGAR; L.ncig = 0; }
  }
  if (L.flag & 4) { L.qlen = 0; L.rlen = 0; }           // bam_set1 measures mapped records only
  if (L.rlen == 0) L.rlen = 1;
  if (cols[F_QUAL].kind == EPI_SIM_STR) {
    L.qual = col_str(cols[F_QUAL], col_elem(cols[F_QUAL], i));
    if (L.qual.n != L.l_seq && L.err == ERR_NONE) L.err = ERR_QUAL;
  } else {
    L.qual = Str{nullptr, 0};
  }
  if (L.err == ERR_NONE) {
    if (L.l_qname > 254) L.err = ERR_QNAME;
    else if (!(L.flag & 4) && L.l_seq > 0 && L.qlen != L.l_seq) L.err = ERR_RECORD;
    else if (L.ncig > 0xFFFF) L.err = ERR_NCIGAR;
  }
  int64_t tb = 0, e;
  for (int t = 0; t < ntags; t++) tb += tag_size(cols[EPI_SIM_NFIELDS + t], i, &e);
  L.tag_bytes = tb;
  L.size = 4 + 32 + (L.l_qname + 1) + 4 * L.ncig + (L.l_seq + 1) / 2 + L.l_seq + tb;
  if (L.size - 4 > 0x7FFFFFFFLL && L.err == ERR_NONE) L.err = ERR_SIZE;
  return L;
}

__global__ __launch_bounds__(256) void k_sim_size(const SimCol *__restrict__ cols, int ntags, int64_t nrecs,
                                                   uint32_t *__restrict__ sizes, uint8_t *__restrict__ err,
                                                   unsigned long long *__restrict__ first_bad) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= nrecs) return;
  const Layout L = record_layout(cols, ntags, i, nullptr);
  sizes[i] = L.err == ERR_NONE ? (uint32_t)L.size : 0u;
  err[i] = L.err;
  if (L.err != ERR_NONE) atomicMin(first_bad, (unsigned long long)i);
}

// byte k of the little-endian value v
__device__ __forceinline__ uint8_t le(uint64_t v, int64_t k) { return (uint8_t)(v >> (8 * k)); }

// Records [r0, r0 + n) of a window: record r0 + x starts at out + off[x].
__global__ __launch_bounds__(256) void k_sim_write(const SimCol *__restrict__ cols, int ntags, int64_t r0, int64_t n,
                                                    uint64_t seed, const uint32_t *__restrict__ off, uint8_t *__restrict__ out) {
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t x = (int64_t)blockIdx.x * kWaves + w;
  if (x >= n) return;
  const int64_t i = r0 + x;
  uint8_t *o = out + off[x];
  const Layout L = record_layout(cols, ntags, i, nullptr);   // every record here has passed k_sim_size
  const int64_t q_at = 36, c_at = q_at + L.l_qname + 1, s_at = c_at + 4 * L.ncig, u_at = s_at + (L.l_seq + 1) / 2,
                t_at = u_at + L.l_seq;
  // block_size refID pos | l_read_name mapq bin | n_cigar_op flag | l_seq next_refID next_pos tlen
  if (lane < 36) {
    const int32_t pos = col_i32(cols[F_POS], i);
    uint32_t v;
    switch (lane >> 2) {
      case 0: v = (uint32_t)(L.size - 4); break;
      case 1: v = (uint32_t)col_i32(cols[F_TID], i); break;
      case 2: v = (uint32_t)pos; break;
      case 3: v = (uint32_t)(L.l_qname + 1) | ((uint32_t)(col_i32(cols[F_MAPQ], i) & 0xFF) << 8) |
                  (reg2bin(pos, (int64_t)pos + L.rlen) << 16); break;
      case 4: v = (uint32_t)L.ncig | ((uint32_t)L.flag << 16); break;
      case 5: v = (uint32_t)L.l_seq; break;
      case 6: v = (uint32_t)col_i32(cols[F_MTID], i); break;
      case 7: v = (uint32_t)col_i32(cols[F_MPOS], i); break;
      default: v = cols[F_ISIZE].kind == EPI_SIM_NONE ? (uint32_t)L.l_seq : (uint32_t)col_i32(cols[F_ISIZE], i); break;
    }
    o[lane] = le(v, lane & 3);
  }
  // read name and its NUL
  const bool own_name = cols[F_QNAME].kind == EPI_SIM_STR;
  for (int64_t b = lane; b <= L.l_qname; b += 64) {
    uint8_t ch;
    if (b == L.l_qname) ch = 0;
    else if (own_name) ch = L.qname.n > 0 ? L.qname.p[b] : (uint8_t)'*';
    else if (b == 0) ch = 'q';
    else {                                                    // sprintf("q%.04i", i + 1)
      int64_t v = L.qname_num;
      for (int64_t k = b; k < L.l_qname - 1; k++) v /= 10;
      ch = (uint8_t)('0' + v % 10);
    }
    o[q_at + b] = ch;
  }
  // CIGAR ops
  if (cols[F_CIGAR].kind == EPI_SIM_STR) {
    if (lane == 0) { int64_t a, b; (void)parse_cigar(L.cigar.p, L.cigar.n, &a, &b, o + c_at); }
  } else if (lane < 4) {
    o[c_at + lane] = le((uint32_t)L.l_seq << 4, lane);
  }
  // bases, two per byte
  const bool rnd = cols[F_SEQ].kind == EPI_SIM_RANDOM;
  for (int64_t m = lane; m < (L.l_seq + 1) / 2; m += 64) {
    const int64_t k = 2 * m;
    const uint32_t hi = nt16(rnd ? random_base(seed, L.seq_j, k) : L.seq.p[k]);
    const uint32_t lo = k + 1 < L.l_seq ? nt16(rnd ? random_base(seed, L.seq_j, k + 1) : L.seq.p[k + 1]) : 0u;
    o[s_at + m] = (uint8_t)((hi << 4) | lo);
  }
  // qualities
  const bool own_qual = cols[F_QUAL].kind == EPI_SIM_STR;
  for (int64_t b = lane; b < L.l_seq; b += 64) o[u_at + b] = own_qual ? (uint8_t)(L.qual.p[b] - 33) : (uint8_t)('F' - 33);
  // tags, in column order
  int64_t at = t_at;
  for (int t = 0; t < ntags; t++) {
    const SimCol &c = cols[EPI_SIM_NFIELDS + t];
    int64_t j;
    const int64_t sz = tag_size(c, i, &j);
    uint8_t *d = o + at;
    if (lane == 0) { d[0] = c.n0; d[1] = c.n1; }
    if (c.kind == EPI_SIM_I32) {
      const uint32_t v = col_u32(c, j);
      if (lane == 2) d[2] = int_tag_type((int32_t)v);
      else if (lane >= 3 && lane < sz) d[lane] = le(v, lane - 3);
    } else if (c.kind == EPI_SIM_F32) {
      if (lane == 2) d[2] = 'f';
      else if (lane >= 3 && lane < 7) d[lane] = le(col_u32(c, j), lane - 3);
    } else if (c.kind == EPI_SIM_STR) {
      const Str v = col_str(c, j);
      for (int64_t b = lane + 2; b < sz; b += 64) d[b] = b == 2 ? (uint8_t)'Z' : b - 3 < v.n ? v.p[b - 3] : (uint8_t)0;
    } else {
      const int64_t e0 = c.offsets[j], cnt = c.offsets[j + 1] - e0;
      const int es = type_size(c.type);
      for (int64_t b = lane + 2; b < sz; b += 64) {
        uint8_t ch;
        if (b == 2) ch = 'B';
        else if (b == 3) ch = c.type;
        else if (b < 8) ch = le((uint64_t)cnt, b - 4);
        else ch = le(col_u32(c, e0 + (b - 8) / es), (b - 8) % es);
        d[b] = ch;
      }
    }
    at += sz;
  }
}

const char *err_text(uint8_t e) {
  switch (e) {
    case ERR_CIGAR: return "Unable to fill CIGAR array";
    case ERR_QUAL: return "Unable to fill BAM record: qual and seq differ in length";
    case ERR_QNAME: return "Unable to fill BAM record: query name longer than 254 bytes";
    case ERR_NCIGAR: return "Unable to fill BAM record: more than 65535 CIGAR operations";
    case ERR_SIZE: return "Unable to fill BAM record: record larger than 2 GiB";
    default: return "Unable to fill BAM record: CIGAR and query sequence are of different length";
  }
}

// sam_hdr_add_lines + bam_hdr_write: the text (the lines, each ended by a newline), then the @SQ sequences
int make_header(const char *const *lines, int32_t nlines, std::vector<uint8_t> &out) {
  std::string text;
  for (int32_t k = 0; k < nlines; k++) {
    if (!lines[k]) return fail(EPI_ERR_ARG, "Unable to init BAM header");
    text += lines[k];
    if (text.empty() || text.back() != '\n') text += '\n';
  }
  std::vector<std::string> names;
  std::vector<int64_t> lens;
  size_t p = 0;
  while (p < text.size()) {
    const size_t e = text.find('\n', p);
    const std::string line = text.substr(p, e - p);
    p = e + 1;
    if (line.compare(0, 4, "@SQ\t") != 0) continue;
    std::string sn;
    int64_t ln = -1;
    size_t f = 4;
    while (f <= line.size()) {
      size_t t = line.find('\t', f);
      if (t == std::string::npos) t = line.size();
      const std::string fld = line.substr(f, t - f);
      if (fld.compare(0, 3, "SN:") == 0) sn = fld.substr(3);
      else if (fld.compare(0, 3, "LN:") == 0) {
        char *end = nullptr;
        ln = strtoll(fld.c_str() + 3, &end, 10);
        if (!end || *end || fld.size() == 3) ln = -1;
      }
      f = t + 1;
    }
    if (sn.empty() || ln < 0 || ln > 0xFFFFFFFFLL) return fail(EPI_ERR_ARG, "Unable to init BAM header: bad @SQ line '%s'", line.c_str());
    names.push_back(sn);
    lens.push_back(ln);
  }
  auto put32 = [&](uint32_t v) { for (int k = 0; k < 4; k++) out.push_back((uint8_t)(v >> (8 * k))); };
  out.clear();
  out.insert(out.end(), {'B', 'A', 'M', 1});
  put32((uint32_t)text.size());
  out.insert(out.end(), text.begin(), text.end());
  put32((uint32_t)names.size());
  for (size_t k = 0; k < names.size(); k++) {
    put32((uint32_t)names[k].size() + 1);
    out.insert(out.end(), names[k].begin(), names[k].end());
    out.push_back(0);
    put32((uint32_t)lens[k]);
  }
  return EPI_OK;
}

bool check_column(const epi_sim_column &c, bool tag) {
  if (c.period < 1) return false;
  if (c.kind == EPI_SIM_NONE) return !tag;
  if (c.len < 1 || !c.values) return false;
  if ((c.kind == EPI_SIM_STR || c.kind == EPI_SIM_ARR) && !c.offsets) return false;
  if (c.kind == EPI_SIM_ARR) return strchr("cCsSiIf", c.type) && c.type;
  return c.kind == EPI_SIM_I32 || c.kind == EPI_SIM_F32 || c.kind == EPI_SIM_STR || c.kind == EPI_SIM_RANDOM;
}

struct SimState {
  std::vector<DevBuf> bufs;
  DevBuf cols, sizes, err, bad, off, scan_tmp, win;
  void *pinned[2] = {nullptr, nullptr};
  std::thread writer;
  ~SimState() {
    if (writer.joinable()) writer.join();                  // first: the writer reads the pinned buffers; the device buffers go after this body
    for (void *p : pinned) if (p) (void)hipHostFree(p);
  }
};

int simulate_impl(epi_engine *eng, const char *out_path, const char *const *lines, int32_t nlines, int64_t nrecs,
                  const epi_sim_column *fields, const epi_sim_column *tags, int32_t ntags, uint64_t seed, int nthreads,
                  int32_t window_kib, int64_t *nwritten) {
  const bool timing = options().bam_timing != 0;
  auto tnow = []() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
  double t_phase[4] = {0, 0, 0, 0}, t_mark = tnow();       // size + check, build, copy, deflate + write (waiting for it)
  auto lap = [&](int k) { const double t = tnow(); t_phase[k] += t - t_mark; t_mark = t; };

  std::vector<uint8_t> header;
  EPI_TRY(make_header(lines, nlines, header));
  EPI_HIP(hipSetDevice(eng->device));
  hipStream_t s = eng->stream;
  SimState S;
  // ---- the columns, at their own lengths ----
  const int ncol = EPI_SIM_NFIELDS + ntags;
  std::vector<SimCol> h_cols((size_t)ncol);
  S.bufs.resize(2 * (size_t)ncol);
  for (int k = 0; k < ncol; k++) {
    const epi_sim_column &c = k < EPI_SIM_NFIELDS ? fields[k] : tags[k - EPI_SIM_NFIELDS];
    SimCol &d = h_cols[(size_t)k];
    memset(&d, 0, sizeof(d));
    d.kind = c.kind; d.type = (uint8_t)c.type; d.len = c.len > 0 ? c.len : 1; d.period = c.period;
    if (k >= EPI_SIM_NFIELDS) { d.n0 = (uint8_t)c.name[0]; d.n1 = (uint8_t)c.name[1]; }
    if (c.kind == EPI_SIM_NONE) continue;
    size_t vbytes = (size_t)c.len * 4;
    if (c.kind == EPI_SIM_STR) vbytes = (size_t)c.offsets[c.len];
    if (c.kind == EPI_SIM_ARR) vbytes = (size_t)c.offsets[c.len] * 4;
    DevBuf &v = S.bufs[2 * (size_t)k];
    EPI_TRY(v.ensure(vbytes));
    if (vbytes) EPI_HIP(hipMemcpyAsync(v.p, c.values, vbytes, hipMemcpyHostToDevice, s));
    d.values = v.as<uint8_t>();
    if (c.offsets) {
      DevBuf &o = S.bufs[2 * (size_t)k + 1];
      EPI_TRY(o.ensure((size_t)(c.len + 1) * 8));
      EPI_HIP(hipMemcpyAsync(o.p, c.offsets, (size_t)(c.len + 1) * 8, hipMemcpyHostToDevice, s));
      d.offsets = o.as<int64_t>();
    }
  }
  EPI_TRY(S.cols.ensure(sizeof(SimCol) * (size_t)ncol));
  EPI_HIP(hipMemcpyAsync(S.cols.p, h_cols.data(), sizeof(SimCol) * (size_t)ncol, hipMemcpyHostToDevice, s));
  // ---- every record sized and checked ----
  std::vector<uint32_t> sizes((size_t)nrecs);
  if (nrecs > 0) {
    const int64_t nblk = (nrecs + 255) / 256;
    EPI_TRY(check_grid(nblk, 256, "simulateBam"));
    EPI_TRY(S.sizes.ensure((size_t)nrecs * 4));
    EPI_TRY(S.err.ensure((size_t)nrecs));
    EPI_TRY(S.bad.ensure(8));
    EPI_HIP(hipMemsetAsync(S.bad.p, 0xFF, 8, s));
    prof_begin("sim_size", s);
    hipLaunchKernelGGL(k_sim_size, dim3((unsigned)nblk), dim3(256), 0, s, S.cols.as<SimCol>(), (int)ntags, nrecs,
                       S.sizes.as<uint32_t>(), S.err.as<uint8_t>(), S.bad.as<unsigned long long>());
    EPI_HIP(hipGetLastError());
    prof_end("sim_size", s);
    unsigned long long bad = 0;
    EPI_HIP(hipMemcpyAsync(&bad, S.bad.p, 8, hipMemcpyDeviceToHost, s));
    EPI_HIP(hipStreamSynchronize(s));
    if (bad != ~0ull) {
      uint8_t e = 0;
      EPI_HIP(hipMemcpy(&e, S.err.as<uint8_t>() + bad, 1, hipMemcpyDeviceToHost));
      return fail(EPI_ERR_ARG, "%s (record %llu)", err_text(e), bad + 1);
    }
    EPI_TRY(copy_to_host(eng, sizes.data(), S.sizes.p, (size_t)nrecs * 4, s));
    EPI_HIP(hipStreamSynchronize(s));
  }
  // ---- windows: whole records, ~window bytes each (a larger record alone) ----
  size_t window = window_kib > 0 ? (size_t)window_kib << 10 : (size_t)64 << 20;
  if (window > ((size_t)1 << 30)) window = (size_t)1 << 30;
  std::vector<int64_t> cut{0};
  size_t widest = 0, acc = 0;
  for (int64_t r = 0; r < nrecs; r++) {
    if (acc > 0 && acc + sizes[(size_t)r] > window) { cut.push_back(r); widest = acc > widest ? acc : widest; acc = 0; }
    acc += sizes[(size_t)r];
  }
  widest = acc > widest ? acc : widest;
  if (nrecs > 0) cut.push_back(nrecs);
  lap(0);
  BgzfWriter out;
  EPI_TRY(out.open(out_path));
  EPI_TRY(out.write(header.data(), header.size(), nthreads));     // its own block, as sam_hdr_write flushes it
  if (nrecs > 0) {
    EPI_TRY(S.win.ensure(widest));
    for (int k = 0; k < 2; k++) EPI_HIP(hipHostMalloc(&S.pinned[k], widest, hipHostMallocDefault));
  }
  int wrc = EPI_OK;                                          // the writer thread's result
  for (size_t wi = 0; wi + 1 < cut.size(); wi++) {
    const int64_t r0 = cut[wi], nw = cut[wi + 1] - r0;
    size_t bytes = 0;
    for (int64_t r = r0; r < r0 + nw; r++) bytes += sizes[(size_t)r];
    EPI_TRY(S.off.ensure((size_t)nw * 4));
    EPI_TRY(scan_exclusive_u32(S.sizes.as<uint32_t>() + r0, S.off.as<uint32_t>(), nw, nullptr, S.scan_tmp, s));
    const int64_t nblk = (nw + kWaves - 1) / kWaves;
    EPI_TRY(check_grid(nblk, 256, "simulateBam"));
    prof_begin("sim_write", s);
    hipLaunchKernelGGL(k_sim_write, dim3((unsigned)nblk), dim3(256), 0, s, S.cols.as<SimCol>(), (int)ntags, r0, nw, seed,
                       S.off.as<uint32_t>(), S.win.as<uint8_t>());
    EPI_HIP(hipGetLastError());
    prof_end("sim_write", s);
    EPI_HIP(hipStreamSynchronize(s));
    lap(1);
    uint8_t *h = static_cast<uint8_t *>(S.pinned[wi & 1]);   // its last reader, the writer of window wi - 2, has been joined
    EPI_HIP(hipMemcpyAsync(h, S.win.p, bytes, hipMemcpyDeviceToHost, s));
    EPI_HIP(hipStreamSynchronize(s));
    lap(2);
    if (S.writer.joinable()) S.writer.join();
    EPI_TRY(wrc);
    lap(3);
    S.writer = std::thread([&out, &wrc, h, bytes, nthreads]() { wrc = out.write(h, bytes, nthreads); });
  }
  if (S.writer.joinable()) S.writer.join();
  EPI_TRY(wrc);
  EPI_TRY(out.close());
  lap(3);
  if (timing)
    fprintf(stderr, "[simulate] size+check %.3f s  build %.3f s  copy %.3f s  deflate+write (waited) %.3f s  windows %zu\n",
            t_phase[0], t_phase[1], t_phase[2], t_phase[3], cut.size() - 1);
  *nwritten = nrecs;
  return EPI_OK;
}

}  // namespace
}  // namespace epi

using namespace epi;

extern "C" int epi_simulate_bam(epi_engine *eng, const char *out_path, const char *const *lines, int32_t nlines, int64_t nrecs,
                                const epi_sim_column *fields, const epi_sim_column *tags, int32_t ntags, uint64_t seed,
                                int nthreads, int32_t window_kib, int64_t *nwritten) {
  if (!out_path || !fields || !nwritten || nrecs < 0 || nlines < 0 || ntags < 0 || (nlines > 0 && !lines) ||
      (ntags > 0 && !tags))
    return fail(EPI_ERR_ARG, "epi_simulate_bam: bad arguments");
  *nwritten = 0;
  for (int k = 0; k < EPI_SIM_NFIELDS; k++) {
    const int kind = fields[k].kind;
    const bool ok = check_column(fields[k], false) &&
                    (k == F_QNAME || k == F_CIGAR || k == F_QUAL ? kind == EPI_SIM_NONE || kind == EPI_SIM_STR
                     : k == F_SEQ ? kind == EPI_SIM_STR || kind == EPI_SIM_RANDOM
                     : k == F_ISIZE ? kind == EPI_SIM_NONE || kind == EPI_SIM_I32 : kind == EPI_SIM_I32);
    if (!ok) return fail(EPI_ERR_ARG, "epi_simulate_bam: bad column for field %d", k);
  }
  for (int k = 0; k < ntags; k++)
    if (!check_column(tags[k], true) || tags[k].kind == EPI_SIM_RANDOM || !tags[k].name || strlen(tags[k].name) != 2)
      return fail(EPI_ERR_ARG, "epi_simulate_bam: bad tag column %d", k);
  if (!eng) EPI_TRY(epi_default_engine(&eng));               // no device: fails here, before any file is touched
  int rc;
  bool created = false;
  try {
    struct stat st;
    created = !(*out_path && stat(out_path, &st) == 0);
    rc = simulate_impl(eng, out_path, lines, nlines, nrecs, fields, tags, ntags, seed, nthreads > 0 ? nthreads : 1,
                       window_kib, nwritten);
  } catch (const std::bad_alloc &) {
    rc = fail(EPI_ERR_NOMEM, "epi_simulate_bam: out of host memory");
  } catch (...) {
    rc = fail(EPI_ERR_STATE, "epi_simulate_bam: unexpected failure");
  }
  if (rc != EPI_OK) {
    *nwritten = 0;
    if (created && *out_path) (void)unlink(out_path);
  }
  return rc;
}
