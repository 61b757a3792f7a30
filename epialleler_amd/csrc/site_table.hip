// The per-strand site table's construction and the host steps every report over it shares (description: site_table.hpp).
#include "site_table.hpp"
#include "cx_table.hpp"

namespace epi {

__global__ __launch_bounds__(SITE_WG) void k_site_strand_flag(const int32_t *__restrict__ strand, uint32_t N, uint32_t *__restrict__ flag) {
  const uint32_t i = blockIdx.x * (uint32_t)SITE_WG + threadIdx.x;
  if (i < N) flag[i] = strand[i] == 1 ? 1u : 0u;
}

__global__ __launch_bounds__(SITE_WG) void k_site_keys(const int32_t *__restrict__ rname, const int32_t *__restrict__ strand,
                                                       const int32_t *__restrict__ pos, const int32_t *__restrict__ context,
                                                       const uint32_t *__restrict__ rank, const uint32_t *__restrict__ n1p, uint32_t N,
                                                       unsigned long long *__restrict__ key, uint8_t *__restrict__ sctx) {
  const uint32_t i = blockIdx.x * (uint32_t)SITE_WG + threadIdx.x;
  if (i >= N) return;
  const uint32_t g = site_ordinal(strand[i], i, rank[i], *n1p);
  if (g >= N) return;
  key[g] = table_key(rname[i], pos[i]);
  sctx[g] = (uint8_t)context[i];
}

uint32_t site_view_args(const epi_batch *b, SiteView &v) {
  const SiteReportState &t = b->sites;
  const int32_t *cx = t.cx.as<int32_t>();
  const size_t N = (size_t)t.nsite;
  v.rname = cx; v.strand = cx + N; v.pos = cx + 2 * N; v.context = cx + 3 * N;
  v.rank = t.rank.as<uint32_t>();
  v.n1 = &t.scalars()->nplus;
  v.key = t.key.as<unsigned long long>();
  v.counts = t.counts.as<uint32_t>();
  return (uint32_t)N;
}

int site_rows(epi_batch *b, const uint32_t *flag, int64_t n, uint32_t *off, uint32_t *total, hipStream_t s, int64_t *count,
              const char *prof) {
  const int rc = scan_exclusive_u32(flag, off, n, total, b->scan_tmp, s);
  if (prof) prof_end(prof, s);
  EPI_HIP(hipGetLastError());
  EPI_TRY(rc);
  // (the reported rows come back with the '+' count in front of them, 8 bytes; blocks and common sites alone, 4)
  SiteScalars *sc = b->sites.scalars();
  const uint32_t *first = total == &sc->nrow ? &sc->nplus : total;
  uint32_t h[2] = {0, 0};
  EPI_TRY(read_scalars(b, s, first, (size_t)(total - first + 1) * 4, h));
  *count = h[total - first];
  return EPI_OK;
}

int site_fetch_begin(const char *who, epi_batch *b, ReportKind kind, const char *what, bool blocks, int32_t *const *icols, int ni,
                     double *const *dcols, int nd, void *stream, hipStream_t *s, int64_t *nrow) {
  *nrow = 0;
  if (!b || !icols || !dcols) return fail(EPI_ERR_ARG, "%s: NULL argument", who);
  if (b->last_kind != kind || (blocks && !b->sites.link.blocks)) return fail(EPI_ERR_STATE, "%s: no finished %s on this batch", who, what);
  const int64_t n = blocks ? b->sites.link.nblock : b->last_nrow;
  if (n == 0) return EPI_OK;
  EPI_TRY(cx_cols_arg(who, icols, ni, dcols, nd));
  EPI_HIP(hipSetDevice(b->eng->device));
  *s = pick_stream(b, stream);
  *nrow = n;
  return EPI_OK;
}

int site_cx_report(epi_batch *b, const char *ctx, hipStream_t s, const char *who, int64_t *nsite) {
  // the un-thresholded CX report of the reported context(s), methylated letters only as in generateCytosineReport (the
  // table has a row per position whose majority is one of them, either case)
  char rep_ctx[8];
  int nrep = 0;
  const uint32_t ctx_mask = ctx_mask_of(ctx);
  for (const char *c = "HXZ"; *c; c++)
    if (ctx_mask & ((1u << ctx_to_idx((unsigned char)*c)) | (1u << (ctx_to_idx((unsigned char)*c) + 8)))) rep_ctx[nrep++] = *c;
  rep_ctx[nrep] = 0;
  *nsite = 0;
  EPI_TRY(epi_batch_cx_report_dev(b, nullptr, rep_ctx, s, nsite));
  const bool whole = b->last_kind == KIND_CX;
  b->last_kind = KIND_NONE;
  if (!whole)
    return fail(EPI_ERR_STATE, "%s: the batch is set up for a sharded report (the sharded form is not built)", who);
  return EPI_OK;
}

int site_cx_fetch(epi_batch *b, int64_t nsite, hipStream_t s, DevBuf &cx) {
  const size_t N = (size_t)nsite;
  EPI_TRY(cx.ensure(N * 6 * 4));
  int32_t *cols[6];
  for (int i = 0; i < 6; i++) cols[i] = cx.as<int32_t>() + (size_t)i * N;
  b->last_kind = KIND_CX;                                  // (for the fetch of the table that has just been made)
  const int rc = epi_batch_cx_fetch_dev(b, cols, s);
  b->last_kind = KIND_NONE;
  return rc;
}

int site_strand_table(epi_batch *b, int64_t nsite, hipStream_t s) {
  const size_t N = (size_t)nsite;
  const int64_t nb_sites = ((int64_t)N + SITE_WG - 1) / SITE_WG;
  EPI_TRY(check_grid(nb_sites, SITE_WG, "heterogeneity site kernels"));
  SiteReportState &t = b->sites;
  EPI_TRY(t.rank.ensure(N * 4));
  EPI_TRY(t.flag.ensure(N * 4));
  EPI_TRY(t.key.ensure(N * 8));
  EPI_TRY(t.sctx.ensure(N));
  EPI_TRY(t.scal.ensure(64));
  const int32_t *cx = t.cx.as<int32_t>();
  uint32_t *nplus = &t.scalars()->nplus;
  uint32_t *flag = t.flag.as<uint32_t>(), *rank = t.rank.as<uint32_t>();
  hipLaunchKernelGGL(k_site_strand_flag, dim3((unsigned)nb_sites), dim3(SITE_WG), 0, s, cx + N, (uint32_t)N, flag);
  EPI_TRY(scan_exclusive_u32(flag, rank, (int64_t)N, nplus, b->scan_tmp, s));
  hipLaunchKernelGGL(k_site_keys, dim3((unsigned)nb_sites), dim3(SITE_WG), 0, s, cx, cx + N, cx + 2 * N, cx + 3 * N, rank, nplus,
                     (uint32_t)N, t.key.as<unsigned long long>(), t.sctx.as<uint8_t>());
  EPI_HIP(hipGetLastError());
  return EPI_OK;
}

int site_table(epi_batch *b, int64_t nsite, hipStream_t s) {
  EPI_TRY(check_grid((nsite + SITE_WG - 1) / SITE_WG, SITE_WG, "heterogeneity site kernels"));
  EPI_TRY(site_cx_fetch(b, nsite, s, b->sites.cx));
  return site_strand_table(b, nsite, s);
}

void site_rows_args(const epi_batch *b, uint32_t ctx_mask, double max_oo, SiteRows &a) {
  a.xm = b->xm; a.off = b->off; a.len = b->len; a.rname = b->rname; a.strand = b->strand; a.start = b->start; a.n = b->n;
  a.key = b->sites.key.as<unsigned long long>(); a.sctx = b->sites.sctx.as<uint8_t>(); a.n1 = &b->sites.scalars()->nplus;
  a.N = (uint32_t)b->sites.nsite;
  ooctx_masks(ctx_mask, &a.oom_mask, &a.oou_mask);
  a.max_oo = max_oo;
}

}  // namespace epi
