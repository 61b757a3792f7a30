// A caller's CX table as the stateless calls (cx_compare.hip, cx_groups.hip, smooth.hip, segment.hip; p_adjust.hip takes a
// column, not a table) see it: the checks of the table and of the output columns as arguments, the device view, and the order
// all of them require of it: rows strictly ascending in (rname, pos, strand).  site_table.hip's fetch checks its columns here too.
#pragma once
#include "common.hpp"

namespace epi {

struct CxTab {                         // a CX table: rname, strand, pos, context, meth, unmeth
  const int32_t *rname, *strand, *pos, *context, *meth, *unmeth;
  uint32_t n;
};

struct CxRowLimit { int64_t rows; const char *text; };             // the most rows a call takes, and how its messages write that
constexpr CxRowLimit kCxMaxRows = {(1LL << 31) - 1, "2^31 - 1"};   // of a table, where a call sets no other limit

// ni int32 and nd double columns of entry point `who`, inputs or outputs: no array and no column is NULL
inline int cx_cols_arg(const char *who, const int32_t *const *icols, int ni, const double *const *dcols, int nd) {
  if ((ni > 0 && !icols) || (nd > 0 && !dcols)) return fail(EPI_ERR_ARG, "%s: NULL argument", who);
  for (int i = 0; i < ni; i++) if (!icols[i]) return fail(EPI_ERR_ARG, "%s: NULL column", who);
  for (int i = 0; i < nd; i++) if (!dcols[i]) return fail(EPI_ERR_ARG, "%s: NULL column", who);
  return EPI_OK;
}

// the row count of a table argument, 0 .. max.rows, and the row capacity of the call's output, where it has one
inline int cx_rows_arg(const char *who, int64_t n, const CxRowLimit &max, int64_t cap = 0) {
  if (n < 0) return fail(EPI_ERR_ARG, "%s: negative row count", who);
  if (cap < 0) return fail(EPI_ERR_ARG, "%s: negative capacity", who);
  return n > max.rows ? fail(EPI_ERR_ARG, "%s: %lld rows, a table holds at most %s", who, (long long)n, max.text) : EPI_OK;
}

// The table argument of entry point `who`: n rows in six columns d, which an empty table need not have.  *t is the view of it.
inline int cx_tab_arg(const char *who, const int32_t *const *d, int64_t n, const CxRowLimit &max, CxTab *t, int64_t cap = 0) {
  *t = CxTab{};
  EPI_TRY(cx_rows_arg(who, n, max, cap));
  if (n == 0) return EPI_OK;
  EPI_TRY(cx_cols_arg(who, d, 6, nullptr, 0));
  *t = CxTab{d[0], d[1], d[2], d[3], d[4], d[5], (uint32_t)n};
  return EPI_OK;
}

// "N rows to write, room for M": the refusal of every call whose rows (`what`: "rows", "regions") outnumber the caller's capacity
inline int cx_rows_fit(const char *who, const char *what, int64_t nrow, int64_t cap) {
  return nrow > cap ? fail(EPI_ERR_ARG, "%s: %lld %s to write, room for %lld", who, (long long)nrow, what, (long long)cap) : EPI_OK;
}

// The scratch of a call that keeps some of n rows (cx_compare.hip's two, smooth.hip's merge), one allocation that goes when the
// call returns: 64 bytes of scalars, `words` u32 per row (keep flags, their scan, ...), the scan's block sums
struct CxKeepScratch : ScratchArena {
  uint32_t *scal, *flag;
  DevBuf scan_tmp;
  int take(int64_t n, int words) {
    const size_t o_scal = reserve(64), o_flag = reserve((size_t)n * 4 * words), o_scan = reserve(scan_tmp_bytes(n));
    uint32_t *scan;
    EPI_TRY(alloc());
    EPI_TRY(at(o_scal, &scal)); EPI_TRY(at(o_flag, &flag)); EPI_TRY(at(o_scan, &scan));
    scan_tmp = DevBuf::view(scan, scan_tmp_bytes(n));
    return EPI_OK;
  }
};

// row i of t against the key (rname, pos, strand): < 0, 0, > 0
__device__ __forceinline__ int cx_cmp(const CxTab &t, uint32_t i, int32_t rname, int32_t pos, int32_t strand) {
  const int32_t r = t.rname[i];
  if (r != rname) return r < rname ? -1 : 1;
  const int32_t p = t.pos[i];
  if (p != pos) return p < pos ? -1 : 1;
  const int32_t s = t.strand[i];
  return s < strand ? -1 : s > strand ? 1 : 0;
}

// row i (i >= 1) is strictly above row i - 1
__device__ __forceinline__ bool cx_above(const CxTab &t, uint32_t i) { return cx_cmp(t, i - 1, t.rname[i], t.pos[i], t.strand[i]) < 0; }

}  // namespace epi
