/*
 * epihip.h -- C ABI of the MI355X-native per-read methylation-call aggregation
 * engine (libepihip.so).  Plain pointers and sizes only; no C++/torch types.
 *
 * The four "drop-in" entry points replace, one for one, the native functions
 * behind the reference's .Call stubs (BBCG/epialleleR v1.13.4):
 *
 *   epi_threshold_reads  <-  rcpp_threshold_reads  src/rcpp_threshold_reads.cpp:15-74
 *                            (.Call "_epialleleR_rcpp_threshold_reads", R/RcppExports.R:64-66)
 *   epi_get_xm_beta      <-  rcpp_get_xm_beta      src/rcpp_get_xm_beta.cpp:10-43
 *                            (.Call "_epialleleR_rcpp_get_xm_beta",     R/RcppExports.R:28-30)
 *   epi_cx_report        <-  rcpp_cx_report        src/rcpp_cx_report.cpp:34-159
 *                            (.Call "_epialleleR_rcpp_cx_report",       R/RcppExports.R:12-14)
 *   epi_mhl_report       <-  rcpp_mhl_report       src/rcpp_mhl_report.cpp:46-228
 *                            (.Call "_epialleleR_rcpp_mhl_report",      R/RcppExports.R:40-42)
 *
 * and, for generateVcfReport (R/generateVcfReport.R, .getBaseFreqReport R/internal.R:611-676):
 *
 *   epi_get_base_freqs   <-  rcpp_get_base_freqs   src/rcpp_get_base_freqs.cpp:15-57
 *                            (.Call "_epialleleR_rcpp_get_base_freqs",  R/RcppExports.R)
 *   epi_fisher_exact     <-  rcpp_fep              src/rcpp_fep.cpp:10-36 (host code)
 *                            (.Call "_epialleleR_rcpp_fep",             R/RcppExports.R)
 *
 * Input layout (what an R/Rcpp shim gathers from the data.frame + seqxm_xptr,
 * see INTEGRATION.md): templates in ROW order (i.e. already sorted by
 * (rname,start) as .readBam leaves them, R/internal.R:193-195):
 *   xm[off[n]]   packed SEQXM bytes, (nt16<<4)|ctx_idx, src/epialleleR.h:28-38
 *   off[n+1]     int64 byte offsets, row x owns xm[off[x] .. off[x+1])
 *   rname[n], strand[n] (1='+',2='-'), start[n] (1-based)   int32, R factor codes
 *   pass[n]      R logical (int32; 0 = FALSE, anything else incl. NA = TRUE)
 *
 * The resident API (epi_batch_*) is the same computation on a batch that stays
 * in HBM between calls -- the analogue of reusing a preprocessBam() object for
 * several reports (R/preprocessBam.R:6-13).
 *
 * Every function returns 0 on success or an EPI_ERR_* code; epi_last_error()
 * gives the message (thread-local).  HIP failures surface this way, never by
 * abort().  There is NO CPU fallback: without the HIP runtime and a gfx950
 * device every compute entry point fails with EPI_ERR_NODEVICE.
 */
#ifndef EPIHIP_H
#define EPIHIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define EPI_OK            0
#define EPI_ERR_ARG       1   /* invalid argument                                   */
#define EPI_ERR_HIP       2   /* HIP runtime error (message has the hipError name)  */
#define EPI_ERR_UNSORTED  3   /* rows not sorted by (rname,start): "PRE-SORTED DATASET IS A REQUIREMENT", rcpp_cx_report.cpp:19 */
#define EPI_ERR_NOMEM     4
#define EPI_ERR_NODEVICE  5   /* no usable GPU                                      */
#define EPI_ERR_STATE     6   /* call sequence error (e.g. fetch before report)     */

const char *epi_last_error(void);
int epi_version(void);

/* Result tables: library-owned host arrays, release with the matching *_free.
 * Factor levels are the reference's: strand {"+","-"}; context
 * c("NA1","CHH","NA3","NA4","NA5","CHG","CG") i.e. 2=CHH 6=CHG 7=CG
 * (rcpp_cx_report.cpp:146-155); rname levels are the caller's. */
typedef struct {
  int64_t nrow;
  int32_t *rname, *strand, *pos, *context, *meth, *unmeth;
} epi_cx_table;

typedef struct {
  int64_t nrow;
  int32_t *rname, *strand, *pos, *context, *coverage;
  double *length, *lmhl;
} epi_mhl_table;

/* (The columns of a table are one allocation: release a table only through these, never column by column.) */
void epi_cx_table_free(epi_cx_table *t);
void epi_mhl_table_free(epi_mhl_table *t);

/* ---- drop-in entry points (host pointers in, host results out) ---------- */

int epi_threshold_reads(const uint8_t *xm, const int64_t *off, int64_t n,
                        const char *ctx_meth, const char *ctx_unmeth,
                        const char *ooctx_meth, const char *ooctx_unmeth,
                        uint32_t min_n_ctx, double min_ctx_meth_frac,
                        double max_ooctx_meth_frac, int32_t *pass_out /* [n] */);

int epi_get_xm_beta(const uint8_t *xm, const int64_t *off, int64_t n,
                    const char *ctx_meth, const char *ctx_unmeth,
                    double *beta_out /* [n] */);

int epi_cx_report(const uint8_t *xm, const int64_t *off, const int32_t *rname,
                  const int32_t *strand, const int32_t *start,
                  const int32_t *pass /* may be NULL = all TRUE */, int64_t n,
                  const char *ctx, epi_cx_table *out);

int epi_mhl_report(const uint8_t *xm, const int64_t *off, const int32_t *rname,
                   const int32_t *strand, const int32_t *start, int64_t n,
                   const char *ctx, int hmax, int hmin, double max_ooctx_meth_frac,
                   epi_mhl_table *out);

/* rcpp_get_base_freqs (src/rcpp_get_base_freqs.cpp:15-57): per VCF site, the bases of the reads that cover it, by
 * strand and pass.  out is the reference's nsite x 20 NumericMatrix, column-major (out[col * nsite + i]); columns
 * U+ACGTN, U-ACGTN, M+ACGTN, M-ACGTN, i.e. col = seq_nt16_int[byte >> 4] + (strand - 1) * 5 + pass * 10 (any code but
 * A, C, G, T -- the 0xF? filler between mates included -- is N).  Sites in the caller's order; site_chr are rname
 * factor codes, INT32_MIN (NA) gives a zero row.  The non-NA sites must be sorted by (code, pos) (the reference's
 * stated precondition, :5): otherwise EPI_ERR_UNSORTED, as for rows out of (rname, start) order.  Rows whose strand
 * is not 1 or 2 count nowhere.  pass may be NULL (all TRUE; NA is TRUE). */
int epi_get_base_freqs(const uint8_t *xm, const int64_t *off, int64_t n, const int32_t *rname, const int32_t *strand,
                       const int32_t *start, const int32_t *pass, const int32_t *site_chr, const int32_t *site_pos,
                       int64_t nsite, double *out /* [20][nsite] */);

/* rcpp_fep (src/rcpp_fep.cpp:10-36): two-sided Fisher exact p-value of each 2x2 table (a[i] b[i] / c[i] d[i]), the
 * tables no more probable than the observed one (relative tolerance 1e-7) summed, clamped at 1.  NA (INT32_MIN) or a
 * negative count in any cell gives NaN (NA_real_).  Host code (no device needed), `nthreads` threads. */
int epi_fisher_exact(const int32_t *a, const int32_t *b, const int32_t *c, const int32_t *d, int64_t n, double *p_out,
                     int nthreads);

/* ---- VCF reader (.readVcf, R/internal.R:230-267: VariantAnnotation::readVcf(info = NA, geno = NA), then expand())
 * Plain, gzip or BGZF text; the fixed columns CHROM POS ID REF ALT only.  One row per ALT allele of every record, in
 * file order, keeping the rows .getBaseFreqReport keeps (R/internal.R:617-620): a one-base REF and a one-character ALT
 * ("." is no allele).  Contigs are numbered in the order of the ##contig header lines, then of first appearance.
 * Names: the ID column, or CHROM:POS_REF/ALT (ALT as written, all alleles) when it is ".". */
typedef struct {               /* library-owned; release with epi_vcf_free */
  int64_t nrec;                /* rows */
  int64_t nrec_file;           /* data lines of the file */
  int32_t n_chrom;
  char **chrom_names;          /* [n_chrom] */
  int32_t *chrom;              /* [nrec] 0-based index into chrom_names */
  int32_t *pos;                /* [nrec] 1-based POS */
  char *ref, *alt;             /* [nrec] one character each */
  char *names;                 /* nrec NUL-terminated names back to back (names_bytes bytes) */
  int64_t names_bytes;
} epi_vcf;
int epi_read_vcf(const char *path, epi_vcf *out);
void epi_vcf_free(epi_vcf *v);

/* ---- genome and methylation calling (preprocessGenome / callMethylation) ------------------------------------------
 * epi_read_genome: a FASTA file (plain, gzip or BGZF; no index needed) -> the sequences in file order.  A name is the
 * header line up to the first whitespace; every byte other than aAcCgGtTnN becomes 'N', lower case becomes upper case;
 * a repeated name is an error.  The object uploads itself to a device the first time a call there needs it and stays
 * resident until epi_genome_free. */
typedef struct epi_genome epi_genome;
int epi_read_genome(const char *path, int nthreads, epi_genome **out);
void epi_genome_free(epi_genome *g);
int32_t epi_genome_count(const epi_genome *g);
const char *epi_genome_name(const epi_genome *g, int32_t i);       /* NULL when i is out of range */
int64_t epi_genome_length(const epi_genome *g, int32_t i);         /* -1 when i is out of range */
const char *epi_genome_sequence(const epi_genome *g, int32_t i);   /* epi_genome_length(g, i) bytes, not NUL-terminated */

/* rcpp_call_methylation_genome + .callMethylation (R/internal.R:405-432): the strand tag (XG, else YD, else ZS) is chosen
 * from the first 1024 records; the header's reference sequences must equal the genome's; every record is written in
 * input order, records that are mapped, carry the strand tag and have no XM get XG (when absent) and XM computed on
 * the GPU.  engine NULL: the default engine.  The output is BGZF written by `nthreads` compressing threads.
 * _windowed: tag "XG" / "YD" / "ZS" forces the strand tag (rcpp_call_methylation_genome's own contract: no check of the
 * first records), NULL chooses it as above; window_kib: inflated bytes per processing window (0: the default), only
 * memory use and batch sizes depend on it. */
int epi_call_methylation(struct epi_engine *eng, const char *in_path, const char *out_path, epi_genome *g, int nthreads,
                         int64_t *nrecs, int64_t *ncalled);
int epi_call_methylation_windowed(struct epi_engine *eng, const char *in_path, const char *out_path, epi_genome *g,
                                  const char *tag, int nthreads, int32_t window_kib, int64_t *nrecs, int64_t *ncalled);

/* ---- simulateBam (rcpp_simulate_bam, R/internal.R:296-403) ----------------------------------------------------------
 * One column of records, as the caller supplied it: record i reads element (i % period) % len, so a short column is
 * recycled on the device and never expanded on the host.  `fields` are always EPI_SIM_NFIELDS columns in this order:
 *   qname (STR, or NONE: "q%04d" of i + 1), flag, tid, pos (0-based), mapq (I32), cigar (STR, or NONE: "<l_seq>M"),
 *   mtid, mpos (0-based), isize (I32, or NONE: l_seq), seq (STR, or RANDOM), qual (STR with '!'-based letters, or NONE:
 *   'F' for every base).
 * RANDOM seq: `values` holds the int32 lengths of the random strings; base k of string j is
 *   "ACTG"[hash3(seed, 0x53494D, (j << 32) | k) >> 62]   (hash3 of synth.hip).
 * Tag columns carry their two-letter `name`; they are written in the order given, with the encodings of HTSlib's
 * bam_aux_update_int (I32: the narrowest of c C s S i I), _float (F32: 'f'), _str (STR: 'Z') and _array (ARR: 'B',
 * subtype `type` of c C s S i I f; `values` int32 elements, or float for 'f', `offsets` the len + 1 element offsets). */
enum { EPI_SIM_NONE = 0, EPI_SIM_I32 = 1, EPI_SIM_F32 = 2, EPI_SIM_STR = 3, EPI_SIM_ARR = 4, EPI_SIM_RANDOM = 5 };
enum { EPI_SIM_NFIELDS = 11 };
typedef struct {
  const char *name;          /* tag columns: the tag's two letters; fields: ignored */
  int32_t kind;              /* EPI_SIM_* */
  char type;                 /* EPI_SIM_ARR: the array subtype */
  const void *values;        /* I32 / RANDOM: int32[len]; F32: float[len]; STR: the bytes; ARR: int32 or float elements */
  const int64_t *offsets;    /* STR: len + 1 byte offsets into values; ARR: len + 1 element offsets; otherwise NULL */
  int64_t len;               /* elements (strings, arrays); >= 1 unless kind is NONE */
  int64_t period;            /* >= 1 */
} epi_sim_column;
/* Writes `nrecs` records after a header made of `lines` (sam_hdr_add_lines: @SQ SN / LN give the reference sequences, in
 * order).  Every record is sized and checked on the GPU before the file is opened, so an invalid call leaves no file;
 * then the records are assembled on the GPU window by window (~64 MiB of uncompressed BAM each, window_kib overrides)
 * and deflated by `nthreads` threads while the next window is built.  engine NULL: the default engine.  Errors use the
 * reference's messages ("Unable to fill CIGAR array", "Unable to fill BAM record", ...) with the failing record. */
int epi_simulate_bam(struct epi_engine *eng, const char *out_path, const char *const *lines, int32_t nlines, int64_t nrecs,
                     const epi_sim_column *fields, const epi_sim_column *tags, int32_t ntags, uint64_t seed, int nthreads,
                     int32_t window_kib, int64_t *nwritten);

/* BGZF writer (host): `n` bytes as blocks of at most 0xff00 input bytes (BC extra field, CRC32), compressed at level 6 by
 * `nthreads` threads and written in order, then the 28-byte end-of-file block. */
int epi_bgzf_write_file(const char *path, const uint8_t *data, int64_t n, int nthreads);

/* ---- host-side producer (preprocessBam) ----------------------------------
 * BAM file -> packed templates sorted by (rname,start), as SoA host buffers (xm in
 * pinned memory when a HIP device is usable).  Replaces rcpp_check_bam
 * (src/rcpp_check_bam.cpp:19-60 + .checkBam, R/internal.R:75-128),
 * rcpp_read_bam_paired / rcpp_read_bam_single (src/rcpp_read_bam.cpp:19-343) and the
 * templid/sort step of .readBam (R/internal.R:154-199) for short-read XG/XM BAMs;
 * BGZF/BAM are decoded with zlib only (no HTSlib).  Same defaults and error
 * conditions as preprocessBam() (R/preprocessBam.R:197-237). */
typedef struct {
  int32_t min_mapq, min_baseq;
  int32_t skip_duplicates, skip_secondary, skip_qcfail, skip_supplementary;   /* R defaults: 0,1,1,1 */
  int32_t trim5, trim3;
  int32_t paired;      /* -1 = detect as .checkBam does; 0/1 = expected endness (error if different) */
  int32_t nthreads;    /* BGZF inflate threads (>=1) */
  /* long-read (MM/ML) alignments only, rcpp_read_bam_mm_single (src/rcpp_read_bam.cpp:364-372): */
  int32_t min_prob;    /* minimum ML probability of a 5mC call (R default -1)                            */
  int32_t highest_prob;/* the 5mC probability must be the highest of all modifications at the base (TRUE) */
  int32_t window_kib;  /* inflated KiB processed per pass (0 = 262144): bounds the host memory next to the output */
} epi_bam_options;

typedef struct {       /* library-owned; release with epi_templates_free */
  int64_t n, nbytes, xm_capacity, nrecs;
  uint8_t *xm;         /* [xm_capacity] packed SEQXM bytes of all templates in row order, 0xFB padded */
  int64_t *off;        /* [n+1] */
  int32_t *rname, *strand, *start;   /* [n] R factor codes / 1-based start */
  int32_t n_targets;
  char **target_names; /* rname levels: all BAM header targets (src/rcpp_read_bam.cpp:173-179) */
  int32_t paired, pinned;
} epi_templates;

int epi_preprocess_bam(const char *path, const epi_bam_options *opt /* NULL = R defaults */, epi_templates *out);
void epi_templates_free(epi_templates *t);

/* preprocessBam with a genome: methylation is called inside the reader, on the GPU, for BAM files that carry only a
 * strand tag (bwa-meth YD, BSMAP ZS, uncalled DRAGEN / Bismark XG).  The contract is the composition
 *     epi_preprocess_bam_genome(eng, in, opt, g, out, &ncalled)
 *         == epi_call_methylation(eng, in, tmp, g, ...) followed by epi_preprocess_bam(tmp, opt, out)
 * with nothing written to disk: the same xm bytes, off, rname, strand, start, target names, paired and nrecs.
 *  - The strand tag (XG, else YD, else ZS) comes from the first 1024 records; a record is called when it is mapped,
 *    carries that tag and has no XM.  Every other record is read as epi_preprocess_bam reads it (a record with XM keeps
 *    its own).  A called record's strand is its XG's first letter, or for YD / ZS input the XG callMethylation would
 *    append ('C': strand 1, 'G': strand 2).
 *  - callMethylation's errors are raised with its messages, before the records concerned are packed: empty file, none
 *    of XG/YD/ZS, header vs genome mismatch, an alignment past its contig's end, a CIGAR that does not consume l_seq
 *    bases, an unknown CIGAR op -- also for records the options would have dropped.  Then epi_preprocess_bam's errors,
 *    with .checkBam's tag flags taken as if the file had been called.
 *  - *ncalled: the number of records callMethylation would have called, whatever the options drop later.
 * engine NULL: the default engine (no device: EPI_ERR_NODEVICE; there is no CPU path).  Without a genome use
 * epi_preprocess_bam, which this leaves unchanged. */
int epi_preprocess_bam_genome(struct epi_engine *eng /* NULL: default */, const char *path,
                              const epi_bam_options *opt /* NULL: R defaults */, epi_genome *g, epi_templates *out,
                              int64_t *ncalled);

/* preprocessBam(mates = "anywhere"): paired-end input whose mates lie anywhere in the file (coordinate-sorted, DRAGEN's
 * default output, or any other order).  The contract is
 *     epi_preprocess_bam_anyorder(eng, F, opt, out)  ==  epi_preprocess_bam(G(F), opt, out)
 * for the xm bytes, off, rname, strand, start, target names, paired and nrecs, where G(F) is F with its records regrouped:
 *  - records with one QNAME form one group; groups appear in the order of each QNAME's first KEPT record in F (kept: none
 *    of the skip flags, 4 and 8 included, flag 2 set, mapq >= min_mapq, usable XG and XM -- what the paired-end packer
 *    uses).  Groups without a kept record produce nothing.  G keeps every record, so nrecs counts all of them.
 *  - within a group, records are ordered by flag & 0xC0 ascending (READ1 before READ2, as samtools sort -n puts them),
 *    ties in their order in F.
 * That fixes the template merge's order: the first record gives rname, start (min(pos, mpos)), width (|isize|) and
 * strand; in an overlap the strictly higher quality wins (a tie keeps the earlier record's byte); the template widens
 * over dovetails and trailing D / N.  Rows with equal (rname, start) keep that order through the stable sort.
 *  - .checkBam's checks come from the first 1024 records of F as in epi_preprocess_bam (paired detection, tags, empty
 *    file, endness), except the name-sorted check, which is skipped.  Single-end and long-read (MM/ML) input gives
 *    exactly epi_preprocess_bam's result.
 *  - Errors carry the messages epi_preprocess_bam gives on G(F); with several bad records another one may be named.
 * Memory: device memory for the kept records' packed inputs (CIGAR ops, one packed byte and one quality per base;
 * allocated once, sized by the file's inflated bytes) plus, while the rows are merged, the output bytes and the
 * per-record and per-template tables; host memory for one window of inflated records (window_kib) plus ~48 bytes per kept
 * record and one QNAME key per template.  The rows are merged on the GPU (assemble_templates.hip).  engine NULL: the
 * default engine (no device: EPI_ERR_NODEVICE before the file is read; there is no CPU path).  Without a genome only. */
int epi_preprocess_bam_anyorder(struct epi_engine *eng /* NULL: default */, const char *path,
                                const epi_bam_options *opt /* NULL: R defaults */, epi_templates *out);

/* ---- report writer (.writeReport, R/internal.R:274-287) -------------------
 * The table as a tab-separated file with a header line, what data.table::fwrite(report, quote=FALSE, sep="\t",
 * col.names=TRUE, compress=if (gzip) "gzip" else "none") writes: integers in decimal, factor columns as their
 * labels, doubles with up to 15 significant digits; NA_integer_ (INT32_MIN), factor codes outside 1..nlevels and
 * NaN are empty fields (na = "").  Rows are formatted by `nthreads` host threads; with gzip != 0 the file is a
 * multi-member gzip file. */
enum { EPI_COL_I32 = 0, EPI_COL_F64 = 1, EPI_COL_FACTOR = 2 };
typedef struct {
  const char *name;            /* header field */
  int32_t kind;                /* EPI_COL_* */
  const void *data;            /* int32_t[nrow] (I32, FACTOR: 1-based codes) or double[nrow] (F64) */
  const char *const *levels;   /* FACTOR: labels */
  int32_t nlevels;
} epi_report_column;
int epi_write_report(const char *path, const epi_report_column *cols, int32_t ncol, int64_t nrow, int32_t gzip,
                     int32_t nthreads);

/* ---- resident API -------------------------------------------------------- */

typedef struct epi_engine epi_engine;   /* one per GPU: device id, streams, pinned staging */
typedef struct epi_batch epi_batch;     /* templates resident in HBM + reusable workspace  */

int epi_engine_create(int device, epi_engine **out);
void epi_engine_destroy(epi_engine *e);
int epi_engine_device(const epi_engine *e);

/* Host SoA -> HBM through two pinned staging buffers and hipMemcpyAsync
 * (double-buffered).  The batch owns its device memory. */
int epi_batch_upload(epi_engine *e, const uint8_t *xm, const int64_t *off,
                     const int32_t *rname, const int32_t *strand, const int32_t *start,
                     int64_t n, epi_batch **out);

/* The same four computations on a batch that is already resident, host results out: what a binding without device
 * memory of its own (the Rcpp shim) calls after ONE epi_batch_upload per preprocessBam()
 * object.  They run on the engine's own stream and return when the results are in the caller's buffers.
 * epi_batch_cytosine_report is generateCytosineReport(threshold.reads=TRUE) in one pass over the bytes
 * (epi_batch_cytosine_report_dev below); pass_out is optional. */
int epi_batch_threshold_reads(epi_batch *b, const char *ctx_meth, const char *ctx_unmeth, const char *ooctx_meth,
                              const char *ooctx_unmeth, uint32_t min_n_ctx, double min_ctx_meth_frac,
                              double max_ooctx_meth_frac, int32_t *pass_out /* [n] */);
int epi_batch_get_xm_beta(epi_batch *b, const char *ctx_meth, const char *ctx_unmeth, double *beta_out /* [n] */);
int epi_batch_cx_report(epi_batch *b, const int32_t *pass /* host, may be NULL = all TRUE */, const char *ctx, epi_cx_table *out);
int epi_batch_cytosine_report(epi_batch *b, const char *ctx_meth, const char *ctx_unmeth, const char *ooctx_meth,
                              const char *ooctx_unmeth, uint32_t min_n_ctx, double min_ctx_meth_frac,
                              double max_ooctx_meth_frac, const char *ctx, int32_t *pass_out /* host, may be NULL */,
                              epi_cx_table *out);
int epi_batch_mhl_report(epi_batch *b, const char *ctx, int hmax, int hmin, double max_ooctx_meth_frac, epi_mhl_table *out);
/* The same reports in two steps, for a binding that owns the result vectors (R's IntegerVector / NumericVector,
 * src/rcpp_cx_report.cpp:133-140, src/rcpp_mhl_report.cpp:200-208): *_begin runs the report on the engine's stream and
 * returns the row count; the caller allocates its columns and epi_batch_cx_fetch_host / epi_batch_mhl_fetch_host (stream
 * NULL) copy the table straight into them -- no library-owned table, no second host copy. */
int epi_batch_cx_report_begin(epi_batch *b, const int32_t *pass /* host, may be NULL */, const char *ctx, int64_t *nrow_out);
int epi_batch_cytosine_report_begin(epi_batch *b, const char *ctx_meth, const char *ctx_unmeth, const char *ooctx_meth,
                                    const char *ooctx_unmeth, uint32_t min_n_ctx, double min_ctx_meth_frac,
                                    double max_ooctx_meth_frac, const char *ctx, int32_t *pass_out /* host, may be NULL */,
                                    int64_t *nrow_out);
int epi_batch_mhl_report_begin(epi_batch *b, const char *ctx, int hmax, int hmin, double max_ooctx_meth_frac, int64_t *nrow_out);
/* the lazily created engine the host-pointer entry points use (device EPIHIP_DEVICE, default 0) */
int epi_default_engine(epi_engine **out);

/* Zero-copy: the caller (e.g. a torch tensor) owns the device buffers, keeps
 * them alive and does not change them while the batch exists.  d_xm must be
 * 16-byte aligned and xm_capacity (bytes allocated) >= off[n] rounded up to
 * 16.  nbytes = off[n].
 * Both constructors queue, on the HIP null stream, one pass over the columns
 * (longest read, (rname,start) order, strand and offset validity): the data
 * must be complete as seen from that stream.  Its verdict is raised by the
 * first report call (EPI_ERR_UNSORTED / EPI_ERR_ARG); per-read functions
 * accept unsorted rows. */
int epi_batch_adopt(epi_engine *e, const uint8_t *d_xm, int64_t xm_capacity, int64_t nbytes,
                    const int64_t *d_off, const int32_t *d_rname, const int32_t *d_strand,
                    const int32_t *d_start, int64_t n, epi_batch **out);
/* Position-congruent rows.  The tile kernels read position-aligned 16-byte chunks; with rows back to back those have
 * any byte alignment and load at ~0.85 of the aligned rate.  epi_batch_realign gives the batch its OWN copy of xm in
 * which row x starts at an offset = start[x] (mod 16) (<= 15 bytes of filler between rows, one pass over the bytes, one
 * host synchronisation) -- the reference keeps one std::string per template (src/epialleleR.h:28-38), so where rows
 * start is the engine's business.  epi_batch_upload does this itself; for an adopted batch it is the caller's call:
 * afterwards the batch no longer reads d_xm / d_off (the caller may free them), and holds B + <= 15 n bytes of its own.
 * Call it before the first report on the batch.  Results never depend on it.  EPIHIP_REALIGN=0 makes it a no-op
 * (A/B runs); 4 / 8 = congruent modulo 4 / 8 only.  epi_batch_layout: 0 = as given, 4 / 16 = congruent modulo that. */
int epi_batch_realign(epi_batch *b, void *stream);
int epi_batch_layout(const epi_batch *b);
/* The rows as the kernels read them: row x owns d_xm[d_off[x] .. d_off[x] + d_len[x]) (d_off: n + 1 non-decreasing
 * entries, d_off[n] = *nbytes; d_len: n; written by a kernel queued on the null stream when the batch was created).
 * Device pointers, valid until the batch is freed or realigned.  Any out-pointer may be NULL. */
int epi_batch_view(const epi_batch *b, const uint8_t **d_xm, const int64_t **d_off, const int32_t **d_len, int64_t *nbytes);
void epi_batch_free(epi_batch *b);
int64_t epi_batch_nrows(const epi_batch *b);

/* `stream` is a hipStream_t; NULL is the HIP null stream (e.g. torch's default
 * stream), so the call is ordered after whatever the caller queued there.  The
 * *_dev functions are asynchronous on that stream unless noted. */
int epi_batch_threshold_reads_dev(epi_batch *b, const char *ctx_meth, const char *ctx_unmeth,
                                  const char *ooctx_meth, const char *ooctx_unmeth,
                                  uint32_t min_n_ctx, double min_ctx_meth_frac,
                                  double max_ooctx_meth_frac, int32_t *d_pass_out, void *stream);
int epi_batch_get_xm_beta_dev(epi_batch *b, const char *ctx_meth, const char *ctx_unmeth,
                              double *d_beta_out, void *stream);

/* rcpp_match_amplicon / rcpp_match_capture (src/rcpp_match_target.cpp:16-81; callers .getBedReport /
 * .getBedEcdf, R/internal.R:529-604): first BED row a read matches, 1-based, or INT32_MIN (NA_integer_).
 * bed_chr are rname factor codes; capture = 0: start or end within `param` (tolerance);
 * capture = 1: overlap >= `param`. */
int epi_batch_match_target_dev(epi_batch *b, const int32_t *d_bed_chr, const int32_t *d_bed_start,
                               const int32_t *d_bed_end, int32_t nbed, int32_t capture, int32_t param,
                               int32_t *d_match_out, void *stream);

/* CX report in two steps so the caller can allocate the output columns:
 *  1) compute: tile index, LDS-histogram tile kernel, majority rule, ordered
 *     row offsets.  Synchronises `stream` (row count comes back to the host).
 *  2) fetch: gathers the rows, in reference order, into six int32 columns of
 *     length nrow in device (fetch_dev, async) or host (fetch_host) memory. */
int epi_batch_cx_report_dev(epi_batch *b, const int32_t *d_pass /* NULL = all TRUE */,
                            const char *ctx, void *stream, int64_t *nrow_out);
/* generateCytosineReport(threshold.reads=TRUE) in one call (R/generateCytosineReport.R:181-199: .thresholdReads, then
 * .getCytosineReport with its result): the same table as epi_batch_threshold_reads_dev followed by
 * epi_batch_cx_report_dev, but the bytes are read from HBM once -- the tile kernel counts the thresholding classes of
 * a read from the registers it already holds and lower-cases the read's calls itself (rcpp_threshold_reads.cpp:28-71,
 * rcpp_cx_report.cpp:118).  Fused for reads of up to ~2.5 kb and class strings without repeated letters; other
 * batches run the two kernels one after the other (same results).  d_pass_out (optional, [n]) receives the pass
 * flags.  Continue with epi_batch_cx_fetch_* (or epi_batch_cx_finish_shared) as after epi_batch_cx_report_dev. */
int epi_batch_cytosine_report_dev(epi_batch *b, const char *ctx_meth, const char *ctx_unmeth, const char *ooctx_meth,
                                  const char *ooctx_unmeth, uint32_t min_n_ctx, double min_ctx_meth_frac,
                                  double max_ooctx_meth_frac, const char *ctx, int32_t *d_pass_out /* may be NULL */,
                                  void *stream, int64_t *nrow_out);
/* The same reports written straight into the caller's six int32 columns of `cap` rows each (rname, strand, pos, context,
 * meth, unmeth).  *written = 1: the columns hold the *nrow_out rows, nothing to fetch.  That happens when every tile
 * is finished inside the tile kernel's launch -- no position of the batch covered by more than 255 rows, not a sharded
 * report -- and the row count recorded by an earlier report on this batch with the same contexts fits `cap`, and every
 * tile yields as many rows as it did then.  For valid XM codes that count does not depend on `pass` or the thresholds;
 * for the low nibbles 1, 3 and 4 (never produced by the packer) a failed read counts differently, and rows rewritten in
 * place may change it: a tile whose count differs makes the call rerun through the row pool (*written = 0) and replaces
 * the record.  *written = 0: as epi_batch_cx_report_dev / epi_batch_cytosine_report_dev; continue with epi_batch_cx_fetch_*.
 * Synchronises `stream` in both cases.  Library-owned memory is never handed out as the report. */
int epi_batch_cx_report_into_dev(epi_batch *b, const int32_t *d_pass /* NULL = all TRUE */, const char *ctx,
                                 int32_t *const d_cols[6], int64_t cap, void *stream, int64_t *nrow_out, int *written);
int epi_batch_cytosine_report_into_dev(epi_batch *b, const char *ctx_meth, const char *ctx_unmeth, const char *ooctx_meth,
                                       const char *ooctx_unmeth, uint32_t min_n_ctx, double min_ctx_meth_frac,
                                       double max_ooctx_meth_frac, const char *ctx, int32_t *d_pass_out /* may be NULL */,
                                       int32_t *const d_cols[6], int64_t cap, void *stream, int64_t *nrow_out, int *written);
/* Capacity query: *nrow = the row count recorded on this batch for the contexts of `ctx` (-1: no record with these
 * contexts).  One record is kept per batch.  A pool report (*written = 0, epi_batch_cx_report_dev, the CX report inside a
 * heterogeneity report) makes it when the batch has none with its contexts, and a direct launch whose tile counts
 * differed replaces it; a pool report that meets a record with its own contexts leaves it as it is.  So the count is that
 * of the report that MADE the record, which need not be the last report with these contexts: under another `pass` the
 * unused low nibbles 1, 3 and 4 give another count, and then the next direct launch reruns through the pool. */
int epi_batch_cx_report_capacity(epi_batch *b, const char *ctx, int64_t *nrow);
int epi_batch_cx_fetch_dev(epi_batch *b, int32_t *const d_cols[6], void *stream);
int epi_batch_cx_fetch_host(epi_batch *b, int32_t *const h_cols[6], void *stream);

int epi_batch_mhl_report_dev(epi_batch *b, const char *ctx, int hmax, int hmin,
                             double max_ooctx_meth_frac, void *stream, int64_t *nrow_out);
int epi_batch_mhl_fetch_dev(epi_batch *b, int32_t *const d_icols[5], double *const d_dcols[2], void *stream);
int epi_batch_mhl_fetch_host(epi_batch *b, int32_t *const h_icols[5], double *const h_dcols[2], void *stream);

/* Heterogeneity report: epipolymorphism (Landan 2012), methylation entropy (Xie 2011) and the fraction of discordant
 * reads (Landau 2014) of every window of k neighbouring sites.  No reference interface is replaced -- the reference has
 * no such report; this one composes two of its rules: the site table of rcpp_cx_report (src/rcpp_cx_report.cpp:58-80,
 * the majority rule) and the read rule of rcpp_mhl_report (src/rcpp_mhl_report.cpp:172-179).
 *  ctx       context letters in both cases, as for the lMHL report ("Zz", "XxZz", ...), k = 2 .. 6 sites per window.
 *  Sites     the rows (rname, strand, pos, context) of the un-thresholded CX report of the whole batch for the upper-case
 *            letters of ctx (pass all TRUE); the row filter below never changes them.  Per (rname, strand) they are
 *            ordered by pos, s_0 < s_1 < ... < s_{m-1}.
 *  Windows   window j (0 <= j <= m - k) is (s_j ... s_{j+k-1}); a window never spans two sequences or strands.
 *  Calls     a row of strand 1 or 2 has a call at a site of its own (rname, strand) when start <= pos < start + length
 *            and the low nibble x of its byte at pos - start has (x & 7) == the site's context code; methylated when
 *            x < 8.  Everything else ('.', '-', another context, a call where there is no site) is no call.
 *  Kept rows the read rule of the lMHL report with hmin = 0: with o_m / o_u the row's methylated / unmethylated calls in
 *            the contexts NOT in ctx, a row is dropped when o_m / (o_m + o_u) > max_ooctx_meth_frac (0 / 0 is NaN: kept).
 *  Counts    a kept row with a call at all k sites of a window adds 1 to counts[window][p], bit i of p set when its call
 *            at the window's i-th site is methylated.  A gap inside a window: nothing for that window.
 *  Metrics   n = sum of the 2^k bins, p_i = counts[i] / n; nreads = n; npatterns = nonzero bins;
 *            beta = sum_p counts[p] popcount(p) / (n k); epipolymorphism = 1 - sum p_i^2;
 *            entropy = -(1 / k) sum_{p_i > 0} p_i log2 p_i; pdr = 1 - (counts[0] + counts[2^k - 1]) / n.
 *            float64, bins summed in ascending order: no launch shape enters a result.
 *  Rows      a window is reported when n >= max(min_reads, 1) and (max_window_span == 0 or
 *            s_{j+k-1} - s_j + 1 <= max_window_span), in the order of the CX rows the windows start on:
 *            (rname, pos of the first site, strand).
 * Two steps as for the lMHL report: report_dev runs the report (synchronises `stream`, the row count comes back), fetch_dev
 * writes the rows into seven int32 columns (rname, strand, pos, end = pos of the last site, context of the first site,
 * nreads, npatterns), four double columns (beta, epipolymorphism, entropy, pdr) and, unless NULL, d_counts [nrow][2^k]
 * int32.  The counters are u32 (n cannot exceed the row count); nsites * 2^k * 4 bytes above 4 GiB: EPI_ERR_ARG before any
 * counter is allocated.  The report runs a CX report of its own first -- epi_batch_cx_report_dev(b, NULL, the
 * upper-case letters of ctx) -- and leaves the direct-mode record (epi_batch_cx_report_capacity) as that call would: a
 * record with those contexts stays as it is, also one made under another `pass`, any other is replaced by this table's.
 * No later report's table depends on it.  Only epi_batch_heterogeneity_fetch_dev may follow the report: it after any
 * other report, or another report's fetch after this one, is EPI_ERR_STATE.  Single GPU only:
 * the counts are additive over row shards once the site table is common, the sharded form is not built (a batch with
 * shared tiles attached: EPI_ERR_STATE). */
int epi_batch_heterogeneity_report_dev(epi_batch *b, const char *ctx, int k, double max_ooctx_meth_frac, int32_t min_reads,
                                       int32_t max_window_span, void *stream, int64_t *nrow_out);
int epi_batch_heterogeneity_fetch_dev(epi_batch *b, int32_t *const d_icols[7], double *const d_dcols[4],
                                      int32_t *d_counts /* may be NULL */, void *stream);

/* The check a heterogeneity report, and a comparison for each of its two sides, makes before it allocates counters:
 * *bytes_out = nsites * 2^k * 4, or EPI_ERR_ARG above 4 GiB, for nsites >= 2^31 or outside 0 <= nsites, 2 <= k <= 6. */
int epi_heterogeneity_counter_bytes(int64_t nsites, int k, int64_t *bytes_out);

/* Heterogeneity comparison: the epiallele histograms of two batches over the windows of the sites both have, and how far
 * the two histograms of a window are apart (the two-sample question of Landan 2012, Landau 2014 and Guo 2017: tumour
 * against normal).  The reference has no such report.  a and b are batches of one engine (else EPI_ERR_ARG); a == b is
 * allowed.  ctx, k (2 .. 6), max_ooctx_meth_frac, calls and kept rows: exactly as for epi_batch_heterogeneity_report_dev.
 *  Common sites  the rows of a's un-thresholded CX report (upper-case letters of ctx, pass all TRUE) for which b's
 *            un-thresholded CX report has a row with the same rname, strand, pos AND context code: a position whose
 *            majority context differs between the two is not common.  rname codes are compared as integers (both
 *            batches under one sequence dictionary).  Per (rname, strand) they are ordered by pos; window j is common
 *            sites j .. j+k-1 of one (rname, strand).  A site of one batch that is not common is ignored by both: it is
 *            neither a gap nor a call, windows span over it.
 *  Counts    counts_a[window][p] from a's kept rows, counts_b[window][p] from b's: the heterogeneity report's rule and bit
 *            order, on the common table.  u32 counters; each of the two arrays is ncommon * 2^k * 4 bytes, above 4 GiB:
 *            EPI_ERR_ARG before any counter is allocated (epi_heterogeneity_counter_bytes).
 *  Rows      a window is reported when n_a >= max(min_reads, 1) and n_b >= max(min_reads, 1) and (max_window_span == 0 or
 *            last - first + 1 <= max_window_span, over the common sites), in the order of a's CX rows the windows start on.
 *  Columns   ten int32: rname, strand, pos, end, context of the first site, nreads_a, nreads_b, npatterns_a,
 *            npatterns_b, df = the bins that are nonzero in counts_a + counts_b, minus 1.  Thirteen double: beta_a, beta_b,
 *            entropy_a, entropy_b, epipolymorphism_a, epipolymorphism_b, pdr_a, pdr_b (the heterogeneity report's
 *            formulas, per batch); delta_beta = beta_b - beta_a; delta_entropy = entropy_b - entropy_a; and with
 *            p_i = counts_a[i] / n_a, q_i = counts_b[i] / n_b, m_i = (p_i + q_i) / 2, bins ascending:
 *            jsd = sum_i [p_i > 0: p_i log2(p_i / m_i) / 2] + [q_i > 0: q_i log2(q_i / m_i) / 2], clamped to [0, 1] (the
 *            Jensen-Shannon divergence in bits); tvd = sum_i |p_i - q_i| / 2; g = 2 sum O ln(O / E) over the nonzero
 *            cells of the 2 x 2^k table, E = (batch total * bin total) / (n_a + n_b), a's bins first, then b's, each
 *            ascending (the likelihood-ratio statistic; with df what a chi-square routine needs -- a p-value is not
 *            computed).  float64, summed by one thread in the stated order: no launch shape enters a result.
 * compare_dev runs both batches' CX reports and the comparison (synchronises `stream`); *ncommon_out = the common sites,
 * *nrow_out = the reported windows.  Fewer than k common sites: an empty report.  compare_fetch_dev writes the columns
 * and, unless NULL, d_counts_a / d_counts_b [nrow][2^k] int32.  State: the comparison lives on a alone.  Only
 * compare_fetch_dev may follow on a: any other fetch on a after the comparison, or compare_fetch_dev after any other
 * report on a, is EPI_ERR_STATE.  b is left without a report (any fetch on b: EPI_ERR_STATE) and holds nothing of the
 * comparison, so a later report on b does not disturb the fetch.  Both batches keep their direct-mode record exactly as
 * epi_batch_cx_report_dev(., NULL, the upper-case letters of ctx) leaves it.  Single GPU only: a batch with shared tiles
 * attached, on either side, is EPI_ERR_STATE. */
int epi_batch_heterogeneity_compare_dev(epi_batch *a, epi_batch *b, const char *ctx, int k, double max_ooctx_meth_frac,
                                        int32_t min_reads, int32_t max_window_span, void *stream, int64_t *ncommon_out,
                                        int64_t *nrow_out);
int epi_batch_heterogeneity_compare_fetch_dev(epi_batch *a, int32_t *const d_icols[10], double *const d_dcols[13],
                                              int32_t *d_counts_a, int32_t *d_counts_b /* either may be NULL */, void *stream);

/* Linkage report: the co-methylation of pairs of neighbouring sites over the reads that cover both, and the methylation
 * haplotype blocks that follow from it (Guo et al. 2017, the paper lMHL comes from).  The reference has no such report.
 *  ctx       context letters in both cases ("Zz", "XxZz", ...); D = max_neighbours, 1 .. 16.
 *  Sites, calls and kept rows: exactly as for the heterogeneity report above -- the rows of the un-thresholded CX report of
 *            the whole batch, ordered by pos per (rname, strand) as s_0 < s_1 < ...; a call where (x & 7) == the site's
 *            context code, methylated when x < 8; the lMHL read rule with hmin = 0 and max_ooctx_meth_frac.
 *  Pairs     pair (j, d) is (s_j, s_{j+d}) for 1 <= d <= D.  A pair never crosses a sequence or strand.
 *  Counts    a kept row with a call at both sites adds 1 to counts[j][d-1][p], p = meth(s_j) + 2 meth(s_{j+d}) (the
 *            heterogeneity report's bit order): the bins are n_uu, n_mu, n_um, n_mm.  What the row shows at the sites in
 *            between does not matter: a '.' or another context between the two is not a gap.  Counters are u32;
 *            nsites * D * 16 bytes above 4 GiB: EPI_ERR_ARG before anything is allocated (epi_linkage_counter_bytes is that
 *            check on its own: the bytes, or EPI_ERR_ARG).
 *  Metrics   float64, from the four integers: n = sum of the bins; margins A = n_mm + n_mu, a = n_um + n_uu,
 *            B = n_mm + n_um, b = n_mu + n_uu; num = n_mm n_uu - n_mu n_um, exact in int64; cov = num / n^2 (n^2 as the
 *            product of two doubles); r2 = num^2 / (A a B b), the product taken left to right in double;
 *            dprime = num / min(A b, a B) when num > 0, num / min(A B, a b) when num < 0, 0 when num == 0.  r2 and dprime
 *            are NaN when any margin is 0.  No launch shape enters a result.
 *  Rows      pair (j, d) is reported when n >= max(min_reads, 1) and (max_distance == 0 or s_{j+d} - s_j <= max_distance),
 *            in the order of the CX row s_j is on, then d ascending.
 *  Columns   eleven int32 (rname, strand, pos, pos2, context of s_j, neighbour = d, nreads, n_uu, n_mu, n_um, n_mm) and
 *            three double (cov, r2, dprime).
 *  Blocks    (epi_batch_linkage_blocks_dev: min_r2 in [0, 1], min_sites >= 2, on the pair table of the last report)  pair
 *            (j, d) is linked when it is reported and r2 >= min_r2; NaN is not linked.  back[e] is the largest
 *            t <= min(D, ordinal of e in its strand) such that the pairs (e - d, d) are linked for every d = 1 .. t.
 *            Blocks are built greedily and do not overlap, per (rname, strand): start at the strand's first site s with
 *            e = s; extend while e + 1 is on the strand and back[e + 1] >= min(D, e + 1 - s); emit (s .. e) when
 *            e - s + 1 >= min_sites; restart at s = e + 1.  Five int32 columns (rname, strand, start, end, nsites) and
 *            one double: mean_r2, the mean of the block's nsites - 1 adjacent (d = 1) r2 values, summed in ascending
 *            site order by one thread.  Block rows are in the order of the CX rows of their first sites.
 * Steps and state as for the heterogeneity report: report_dev runs the report (synchronises `stream`), fetch_dev writes the
 * rows.  blocks_dev and the two linkage fetches are valid only after a linkage report (blocks_fetch_dev only after
 * blocks_dev on it); any other report's fetch after a linkage report, or a linkage fetch after any other report, is
 * EPI_ERR_STATE.  blocks_dev does not invalidate the pair table, and may be repeated with other arguments.  The CX report
 * inside leaves the direct-mode record exactly as epi_batch_cx_report_dev(b, NULL, the upper-case letters of ctx) would.
 * Single GPU only: the counts are additive over row shards once the site table is common, the sharded form is not built
 * (a batch with shared tiles attached: EPI_ERR_STATE). */
int epi_batch_linkage_report_dev(epi_batch *b, const char *ctx, int max_neighbours, int32_t max_distance,
                                 double max_ooctx_meth_frac, int32_t min_reads, void *stream, int64_t *nrow_out);
int epi_batch_linkage_fetch_dev(epi_batch *b, int32_t *const d_icols[11], double *const d_dcols[3], void *stream);
int epi_batch_linkage_blocks_dev(epi_batch *b, double min_r2, int32_t min_sites, void *stream, int64_t *nblock_out);
int epi_batch_linkage_blocks_fetch_dev(epi_batch *b, int32_t *const d_icols[5], double *const d_dcols[1], void *stream);
int epi_linkage_counter_bytes(int64_t nsites, int max_neighbours, int64_t *bytes_out);

/* FDRP report: the fraction of discordant read pairs (FDRP) and its quantitative form (qFDRP, the mean normalised Hamming
 * distance of read pairs) per cytosine, the two within-sample heterogeneity scores of the WSH package (Scherer et al.
 * 2020).  The reference has no such report.  Where every other score of this family is a sum over reads, these are sums
 * over PAIRS of reads that cover a site.
 *  ctx       context letters in both cases ("Zz", "XxZz", ...), as for the lMHL report; W = flank_sites, 0 .. 31;
 *            m = max_reads, 2 .. 64; min_overlap, 1 .. 2W + 1; max_distance >= 0; max_ooctx_meth_frac and min_reads as for
 *            the heterogeneity report.  Anything out of range: EPI_ERR_ARG before any work.
 *  Sites, calls and kept rows: exactly as for the heterogeneity report above -- the rows of the un-thresholded CX report of
 *            the whole batch, ordered by pos per (rname, strand); a call where (x & 7) == the site's context code,
 *            methylated when x < 8; the lMHL read rule with hmin = 0 and max_ooctx_meth_frac.
 *  Coverage  c of site g = the kept rows with a call at g.
 *  Selection the rows that cover g, listed in ascending batch row index: all of them when c <= m, otherwise the m rows at
 *            ranks floor(j c / m), j = 0 .. m - 1, of that list (the product in 64 bits).  nreads = min(c, m).  The choice is
 *            deterministic, spread over the whole list, and depends on neither launch shape nor atomic order.
 *  Window    of g: the sites g - W .. g + W of g's (rname, strand) segment of the table, clipped at the segment's ends; with
 *            max_distance > 0 only those whose position is within max_distance bases of g's.  g itself is always in it.
 *  Pairs     (a, b) of used rows, a < b in list order.  o = the window sites at which both rows have a call (o >= 1: both
 *            call g), h = those of them at which the two calls differ.  The pair counts when o >= min_overlap; then
 *            npairs += 1, ndiscordant += (h > 0), H[o] += h.
 *  Scores    float64: fdrp = ndiscordant / npairs; qfdrp = (sum over o = 1 .. 2W + 1 of H[o] / o) / npairs, every integer
 *            H[o] divided by o and the terms added in ascending o by one thread.  No launch shape enters a result: a
 *            restatement that performs the same IEEE operations in the same order agrees bit for bit.
 *  Rows      a site is reported when nreads >= max(min_reads, 2) and npairs >= 1, in CX row order.
 *  Columns   eight int32 (rname, strand, pos, context, coverage, nreads, npairs, ndiscordant) and two double (fdrp, qfdrp).
 * Two deviations from WSH are deliberate.  The reads of a deep site are SELECTED DETERMINISTICALLY (evenly spaced ranks)
 * where WSH draws 40 at random: a report is reproducible.  And two reads are compared over a WINDOW OF SITES around the
 * cytosine where WSH compares them over their whole overlap in bases: with long reads the whole overlap makes nearly every
 * pair discordant, and the score of a site would depend on the read length.
 * Steps and state as for the heterogeneity report: report_dev runs the report (synchronises `stream`), fetch_dev writes the
 * rows.  Only epi_batch_fdrp_fetch_dev may follow the report: it after any other report, or another report's fetch after
 * this one, is EPI_ERR_STATE.  The CX report inside leaves the direct-mode record exactly as
 * epi_batch_cx_report_dev(b, NULL, the upper-case letters of ctx) would.  The report lists one (site, row) pair per call
 * of a kept row and sorts the list by site; the list holds fewer than 2^32 pairs (the sort's indices are 32-bit), more is
 * EPI_ERR_ARG before the list is allocated.  epi_fdrp_pair_bytes is that check on its own: *bytes_out = the bytes of the
 * two (key, row) buffers, 24 per call, or EPI_ERR_ARG for ncalls < 0 or ncalls >= 2^32.  Single GPU only: the sharded form
 * is not built (a batch with shared tiles attached: EPI_ERR_STATE). */
int epi_batch_fdrp_report_dev(epi_batch *b, const char *ctx, int flank_sites, int max_reads, int min_overlap, int32_t max_distance,
                              double max_ooctx_meth_frac, int32_t min_reads, void *stream, int64_t *nrow_out);
int epi_batch_fdrp_fetch_dev(epi_batch *b, int32_t *const d_icols[8], double *const d_dcols[2], void *stream);
int epi_fdrp_pair_bytes(int64_t ncalls, int64_t *bytes_out);

/* Region report: read-level statistics per region of a list -- the methylated haplotype load of Guo et al. 2017 and the
 * per-interval metrics of the mHap tool-chain (mean methylation, PDR, CHALM, MCR, MBS) with the U / X / M read fractions.
 * The reference has no such report.  The other read-level reports are keyed by a cytosine or a window of k cytosines; this
 * one is keyed by the caller's regions: d_chr / d_start / d_end are nregions device int32 (rname factor codes, 1-based
 * closed ranges), in any order, overlapping and repeated as the caller likes; a code no row has (INT32_MIN for NA) gives a
 * row of zero counts.
 *  ctx       context letters in both cases, as for the lMHL report.  1 <= min_sites <= max_sites <= 256;
 *            reverse_offset >= 0; 0 <= u_max < m_min <= 1.  Anything out of range, or a NULL pointer: EPI_ERR_ARG with a
 *            message that names the argument, before any work.
 *  Kept rows the lMHL read rule with hmin = 0 and max_ooctx_meth_frac over the whole row, as for the heterogeneity report.
 *  Calls     of a kept row x in region [start, end] on its rname: its bytes whose context code is one of ctx's and whose
 *            position start[x] + i - (strand[x] == 2 ? reverse_offset : 0) lies in [start, end], in row order; n of them,
 *            m methylated (codes 2, 5, 6, 7), r_1 .. r_q the lengths of the maximal runs of methylated calls.  The row is
 *            counted when 1 <= n <= max_sites and a k-read when also n >= min_sites.
 *  Columns   one row per region, in input order.  Fifteen int32: rname, start, end (as given), nreads (rows with n >= 1),
 *            nlong (rows with n > max_sites: in nreads and nowhere else), kreads, tbase = sum n, mbase = sum m, cbase =
 *            sum (n - m) over rows with m >= 1 (the three over counted rows), ndiscordant (k-reads with 0 < m < n),
 *            nmethylated (k-reads with m >= 1), n_u (k-reads with (double)m <= u_max * (double)n), n_x, n_m (of the rest,
 *            those with (double)m >= m_min * (double)n; n_x is what remains), maxsites (the largest n of a counted row).
 *            Six double: beta = mbase / tbase, pdr = ndiscordant / kreads, chalm = nmethylated / kreads, mcr = cbase / tbase,
 *            mbs = (sum_{n = min_sites}^{maxsites} S2[n] / (n n)) / kreads in ascending n, S2[n] = sum over k-reads with n sites
 *            of sum_j r_j^2, and mhl = (sum_{l = 1}^{maxsites} l (M[l] / T[l])) / (sum_{l = 1}^{maxsites} l) in ascending l,
 *            M[l] = sum over counted rows and runs of max(0, r_j - l + 1), T[l] = sum over counted rows of max(0, n - l + 1).
 *            Every sum is an integer, every ratio one fp64 evaluation per region in the order written (csrc/region_report.hip
 *            has the definitions in full); a zero denominator gives NaN.  The device counts in 64 bits: a count above
 *            2^31 - 1 is EPI_ERR_ARG with the region's index, not a wrapped number.
 * The call is stateless with respect to the batch: it writes the caller's columns, keeps nothing, and its scratch goes with
 * it on every return path (epi_device_allocations reads the same before and after).  It needs no other report and disturbs
 * none.  The rows must be sorted by (rname, start): otherwise EPI_ERR_UNSORTED, and nothing is written.  nregions == 0:
 * EPI_OK, nothing is touched; an empty batch: every region gets its row of zeros.  Synchronises `stream` twice (the
 * candidate rows of the regions; the overflow verdict).  Memory: consecutive regions form a group while their counters and
 * bookkeeping stay under 256 MiB (test hook EPIHIP_RGN_GROUP_BYTES; a region above the cap runs alone);
 * epi_region_counter_bytes gives the counters of nregions regions, nregions * (3 max_sites + 16) * 8, or EPI_ERR_ARG outside
 * 0 <= nregions < 2^31, 1 <= max_sites <= 256.  Single GPU only: the counters are additive over row shards, the sharded form
 * is not built. */
int epi_batch_region_report_dev(epi_batch *b, const int32_t *d_chr, const int32_t *d_start, const int32_t *d_end, int32_t nregions,
                                const char *ctx, int32_t min_sites, int32_t max_sites, int32_t reverse_offset,
                                double u_max, double m_min, double max_ooctx_meth_frac,
                                int32_t *const d_icols[15], double *const d_dcols[6], void *stream);
int epi_region_counter_bytes(int64_t nregions, int32_t max_sites, int64_t *bytes_out);

/* M-bias report: methylation by offset from either end of the template, per strand and context -- the table a user reads
 * preprocessBam's `trim` off -- and the totals per strand and context over every byte, whose non-CpG part is the usual
 * estimate of the bisulfite conversion.  The reference has no such report.
 *  Definition (all integers).  Row x has strand s = strand[x] in {1, 2}, length L = len[x] and bytes b_0 .. b_{L-1} with
 *            codes c_i = b_i & 15.  A code has a class when it is one of
 *              7 (CG, methylated), 15 (CG, unmethylated), 6 (CHG, methylated), 14 (CHG, unmethylated), 2 (CHH, methylated),
 *              10 (CHH, unmethylated);
 *            every other code (5, 13, the filler 11, '.' 12 and the unused ones) has no class and counts nowhere.  For every
 *            byte i that has a class:
 *              totals[s][ctx][state] += 1                                (once per byte, whatever max_offset is)
 *              if i < max_offset:         start[s][ctx][i][state] += 1
 *              if L - 1 - i < max_offset: end[s][ctx][L - 1 - i][state] += 1
 *            A byte of a row shorter than 2 max_offset may count in both tables.  Offsets are template (reference-spaced)
 *            coordinates, filler included -- the coordinates trim cuts in: trim5 = t removes exactly the offsets < t of the
 *            start table, trim3 likewise of the end table.  There is no read rule, no thresholding and no majority rule:
 *            every row counts, and the rows need not be sorted.
 *  Outputs   1 <= max_offset <= 1024.  d_counts: 2 * 2 * 3 * max_offset * 2 device int64, indexed
 *            ((((e * 2 + (s - 1)) * 3 + k) * max_offset + d) * 2 + state), e = 0 for start and 1 for end, k = 0, 1, 2 for the
 *            context codes 2 (CHH), 6 (CHG), 7 (CG), d the offset, state = 0 for methylated and 1 for unmethylated.  d_totals:
 *            12 device int64, indexed (((s - 1) * 3 + k) * 2 + state).
 * A NULL batch or output, or max_offset out of range: EPI_ERR_ARG with a message that names the argument, before any work;
 * nothing is written.  A strand outside {1, 2} on a row with bytes, or bad offsets: EPI_ERR_ARG as the cytosine report raises
 * them, nothing written.  An empty batch: both arrays are zeroed, EPI_OK.  The call is stateless with respect to the batch: it
 * writes the caller's arrays, keeps nothing and disturbs no other report's state (tile index, kept cell lists, site table,
 * allele pairs); its scratch -- per workgroup (at most 1024) 24 max_offset u32 cells and twelve u64 totals, 14 MiB at
 * max_offset = 150 and 96 MiB at 1024 -- goes with it on every return path (epi_device_allocations reads the same before and
 * after).  Synchronises `stream` once, at its end.  Sums of integers: the result is the same from run to run.  Single GPU only:
 * the counters are additive over row shards, so the sharded form is a sum; it is not built.  (csrc/mbias.hip has the data path.) */
int epi_batch_mbias_report_dev(epi_batch *b, int32_t max_offset, int64_t *d_counts, int64_t *d_totals, void *stream);

/* Allele-specific methylation report: does methylation differ between the two alleles of a heterozygous SNV?  Per (SNV,
 * cytosine) the calls of the reads that carry the reference allele against those of the reads that carry the alternative
 * one, with a Fisher exact test, and the same pooled per SNV (what CGmapTools asm, MethPipe allelicmeth and DAMEfinder's SNP
 * mode report).  The reference has no such report.  The packed byte holds the base (nt16 << 4) next to the call, so a row
 * says both which allele it carries and what it calls.
 *  Inputs    a resident batch; nsite sites as device int32 d_site_chr (rname factor codes, INT32_MIN = NA), d_site_pos
 *            (1-based) and d_site_alleles.  The sites are sorted by (code, pos), equal keys allowed (multi-ALT records) and NA
 *            codes (which sort first) included: the precondition of epi_batch_base_freqs_dev, and its EPI_ERR_UNSORTED.
 *  Alleles   d_site_alleles packs four 4-bit masks over the bases A, C, G, T (bit = seq_nt16_int, 0 .. 3): bits 0-3 REF on
 *            '+' rows, 4-7 ALT on '+', 8-11 REF on '-', 12-15 ALT on '-' -- bisulfite-aware, so C>T reads as REF = C, ALT = T
 *            on '-' and as nothing on '+'.  A zero mask: the strand cannot tell the alleles apart.  A bit above 15, or REF
 *            and ALT of one strand sharing a bit: EPI_ERR_ARG naming the site, before any counting.
 *  Kept rows the lMHL read rule with hmin = 0 and max_ooctx_meth_frac over the whole row, as for the heterogeneity and
 *            region reports; the strand must be 1 or 2, the length positive.
 *  Allele    a kept row x covers site s when rname[x] == site_chr[s] and start[x] <= site_pos[s] <= start[x] + len[x] - 1 (no
 *            row covers an NA site).  Its base there is seq_nt16_int[byte >> 4]; its allele is 0 when the base's bit is in its
 *            strand's REF mask, 1 when in the ALT mask, none otherwise (N, the 0xF? filler between mates, a third base, an
 *            uninformative strand).
 *  Events    for a covering row with an allele, every byte of the row whose context code is one of ctx's (letters in both
 *            cases, as for the lMHL report), at position q = start[x] + i with q != site_pos[s] and, when max_distance > 0,
 *            |q - site_pos[s]| <= max_distance (0: no limit, as in the linkage report): one event (s, strand, q, context code =
 *            code & 7, allele, methylated = codes 2, 5, 6, 7).
 *  Pair rows events grouped by (s, q, strand, context code), four cells meth_ref, unmeth_ref, meth_alt, unmeth_alt; reported
 *            when meth_ref + unmeth_ref >= max(min_coverage, 1) and the same holds for alt, in ascending (s, q, strand,
 *            context).  Ten int32 columns: snv (index into the site list as given), rname, snv_pos, strand, pos, context and
 *            the four cells.  Four double: beta_ref, beta_alt (one IEEE division of integers each), delta_beta = beta_alt -
 *            beta_ref, p = the two-sided Fisher p-value of (meth_ref unmeth_ref / meth_alt unmeth_alt) as
 *            epi_fisher_exact_dev computes it, one thread per row.
 *  SNV rows  one per site, in input order.  Ten int32: rname, pos (as given), reads_ref, reads_alt, reads_other (kept covering
 *            rows by allele / without one), npairs (the site's reported pair rows), meth_ref, unmeth_ref, meth_alt, unmeth_alt
 *            summed over the site's REPORTED pair rows (the SNV table is a group-by of the pair table).  Four double: beta_ref,
 *            beta_alt, delta_beta and p from the pooled cells; a zero denominator gives NaN (p of an all-zero table is 1).  An
 *            NA site: zero counts, four NaN.  The device sums in 64 bits: a sum above 2^31 - 1 is EPI_ERR_ARG with the site's
 *            index.  (csrc/asm_report.hip has the definitions in full.)
 * epi_batch_asm_report_dev writes the SNV columns and *npair_out and keeps the pair table on the batch in a state of its own:
 * it touches neither last_kind nor any other report's state, so a CX, lMHL, heterogeneity, linkage or FDRP report fetched
 * after it reads what it read before; the table goes with the batch (epi_device_allocations reads the same after
 * epi_batch_free as before the upload) and the call's scratch on every return path.  epi_batch_asm_fetch_dev writes the pair
 * table's columns (*npair_out rows each); before any report: EPI_ERR_STATE.  nsite == 0: EPI_OK and an empty pair table; an
 * empty batch: zero pair rows and SNV rows of zero counts.  Rows not sorted by (rname, start): EPI_ERR_UNSORTED, nothing
 * written.  max_distance < 0, min_coverage < 0, nsite outside 0 .. 2^31 - 1 or a NULL pointer: EPI_ERR_ARG naming the argument,
 * before any work.  The report synchronises `stream` (site checks, event counts, once per group of sites, overflow verdict).
 * Memory: consecutive sites form a group while their events, 24 bytes each with the sort's second buffers, stay under 256 MiB
 * (test hook EPIHIP_ASM_GROUP_BYTES; a site above the cap runs alone; a single site with more than 2^31 - 1 events is
 * EPI_ERR_ARG); epi_asm_event_bytes gives the bytes of nevents events, 24 nevents, or EPI_ERR_ARG outside 0 <= nevents < 2^32.
 * Single GPU only: the cells are additive over row shards, the sharded form is not built. */
int epi_batch_asm_report_dev(epi_batch *b, const int32_t *d_site_chr, const int32_t *d_site_pos, const int32_t *d_site_alleles,
                             int64_t nsite, const char *ctx, int32_t max_distance, int32_t min_coverage, double max_ooctx_meth_frac,
                             int32_t *const d_snv_icols[10], double *const d_snv_dcols[4], void *stream, int64_t *npair_out);
int epi_batch_asm_fetch_dev(epi_batch *b, int32_t *const d_icols[10], double *const d_dcols[4], void *stream);
int epi_asm_event_bytes(int64_t nevents, int64_t *bytes_out);

/* epi_fisher_exact on the device: d_p[i] = the two-sided Fisher exact p-value of the table (d_a[i] d_b[i] / d_c[i] d_d[i]),
 * by the definition and the arithmetic of epi_fisher_exact (csrc/fisher_math.hpp is compiled into both): P(k) in Loader's
 * saddle-point form, a table as extreme when P(k) <= P(a) (1 + 1e-7), the tails found by bisection and summed outwards by
 * the ratio recurrence until a term no longer changes the sum, the result clamped at 1; a negative cell (NA included): NaN;
 * degenerate margins (one table only): exactly 1.0.  One thread per table performs the host's operations in the host's
 * order, so no launch shape enters a result; against the host the results differ by what the device's lgamma / log / exp
 * differ from the host's (a few ulp, scaled by the size of the exponent).  All pointers are device memory of e's device;
 * the kernel is queued on `stream`, nothing is synchronised.  n == 0: nothing is done. */
int epi_fisher_exact_dev(epi_engine *e, const int32_t *d_a, const int32_t *d_b, const int32_t *d_c, const int32_t *d_d,
                         int64_t n, double *d_p, void *stream);

/* Cytosine report comparison: two CX tables against each other per cytosine (tumour against normal), and the regions over
 * which they differ.  The reference has no such report.  Both calls are stateless: they read device columns of the caller,
 * write device columns of the caller, hold their scratch for the length of the call and touch no batch and no batch's
 * report state.  Both synchronise `stream`.
 *  Inputs    d_a (na rows), d_b (nb rows): CX tables as epi_batch_cx_fetch_dev writes them (rname, strand, pos, context,
 *            meth, unmeth), thresholded or not, of any batches of e's device.  rname codes are compared as integers (both
 *            tables under one sequence dictionary).  Precondition, checked on the device: the rows of each table strictly
 *            ascend in (rname, pos, strand) -- the CX row order whenever the batch's rname codes ascend.  Otherwise
 *            EPI_ERR_ARG, and nothing is written.
 *  Common    a row of a is common when b has a row with the same rname, strand, pos AND context code (the rule of
 *            epi_batch_heterogeneity_compare_dev: a position whose majority context differs is not common).
 *            *ncommon_out = their number.
 *  Rows      a common site is reported when meth_a + unmeth_a >= max(min_coverage, 1) and meth_b + unmeth_b >=
 *            max(min_coverage, 1), in a's row order.  *nrow_out = their number.
 *  Columns   eight int32: rname, strand, pos, context, meth_a, unmeth_a, meth_b, unmeth_b.  Four double: beta_a = meth_a /
 *            (meth_a + unmeth_a), beta_b likewise (one IEEE division of integers each), delta_beta = beta_b - beta_a, p = the
 *            two-sided Fisher p-value of (meth_a unmeth_a / meth_b unmeth_b) as epi_fisher_exact_dev computes it.
 *  Capacity  the columns hold `cap` rows.  cap < *nrow_out: EPI_ERR_ARG, nothing is written, *nrow_out is the count
 *            needed.  cap >= min(na, nb) always suffices.  na == 0 or nb == 0: an empty report.
 *  Regions   (epi_cx_compare_regions_dev, on the n rows of such a table; max_p and min_delta_beta in [0, 1], max_gap >= 0,
 *            min_sites >= 1, else EPI_ERR_ARG)  row i is significant when p[i] <= max_p and |delta_beta[i]| >= min_delta_beta
 *            and delta_beta[i] != 0; NaN is never significant; its direction is the sign of delta_beta.  A region is a
 *            maximal run of consecutive table rows, both strands in table order, that are all significant, of one direction
 *            and one rname, with pos[i + 1] - pos[i] <= max_gap between neighbours; a row that is not significant ends the
 *            run.  Runs of at least min_sites rows are reported, in table order.  Five int32: rname, start = pos of the
 *            first row, end = pos of the last, nsites, direction (+1: b above a, -1).  Five double: beta_a and beta_b pooled
 *            as sum(meth) / sum(meth + unmeth) with 64-bit integer sums, delta_beta = pooled b - a, mean_delta_beta = the
 *            mean of the rows' delta_beta, summed in ascending row order by one thread, p = the Fisher test of the pooled
 *            table (64-bit cells).  Capacity as above (*nregion_out: the count needed).  Neither call adjusts a p-value for
 *            the number of tests: epi_p_adjust_dev (below) does that, for a table's p column or a region table's. */
int epi_cx_compare_dev(epi_engine *e, const int32_t *const d_a[6], int64_t na, const int32_t *const d_b[6], int64_t nb,
                       int32_t min_coverage, int32_t *const d_icols[8], double *const d_dcols[4], int64_t cap,
                       void *stream, int64_t *ncommon_out, int64_t *nrow_out);
int epi_cx_compare_regions_dev(epi_engine *e, const int32_t *const d_icols[8], const double *const d_dcols[4], int64_t n,
                               double max_p, double min_delta_beta, int32_t max_gap, int32_t min_sites,
                               int32_t *const d_ricols[5], double *const d_rdcols[5], int64_t cap, void *stream,
                               int64_t *nregion_out);

/* Multiple-testing correction of a column of p-values on the device: R's p.adjust without `hommel`.  The reference has no
 * such call.  Stateless, like epi_cx_compare_dev: it reads and writes device columns of the caller, holds its scratch
 * (about 24 bytes per row for the sort's two buffers and 8 bytes per row of terms) for the length of the call, touches no
 * batch and synchronises `stream`.
 *  Values    d_p holds n doubles.  NaN is NA: the row is not a test and its q is NaN.  -0.0 counts as 0.0.  Any other value
 *            outside [0, 1] (negative, above 1, +-inf): EPI_ERR_ARG, and nothing is written; the check runs on the device.
 *            m = the number of values that are not NaN, returned in *nvalid_out.  N = n_tests when n_tests > 0, and then
 *            n_tests >= m, else EPI_ERR_ARG (R's p.adjust(n =)); otherwise N = m.  n == 0 or m == 0: nothing is computed, q
 *            is all NaN.  n >= 2^31 or n_tests >= 2^31: EPI_ERR_ARG.  d_q == d_p (in place) is allowed.
 *  Order     d_order (may be NULL) receives n entries: d_order[r] is the row with ascending rank r, in the stable ascending
 *            order of p with NaN last -- numpy's argsort(p, kind="stable").
 *  Methods   s_r: the r-th smallest valid p, r = 1 .. m.  All arithmetic is fp64, each term in exactly this operation order:
 *              EPI_PADJ_NONE        t_r = s_r
 *              EPI_PADJ_BONFERRONI  t_r = N * s_r
 *              EPI_PADJ_HOLM        t_r = max over j <= r of (N + 1 - j) * s_j
 *              EPI_PADJ_HOCHBERG    t_r = min over j >= r of (N + 1 - j) * s_j
 *              EPI_PADJ_BH          t_r = min over j >= r of (N / j) * s_j
 *              EPI_PADJ_BY          t_r = min over j >= r of ((c * N) / j) * s_j, c = the sum over k = 1 .. N of 1.0 / k,
 *                                   summed in ascending k in fp64 by this function on the host, once per call
 *            and q = min(1, t_r), written to the row the rank came from.  N + 1 - j is an integer, converted exactly; every
 *            term is one correctly rounded division and / or multiplication (the library is built without fast-math and
 *            without contraction), minimum and maximum are exact: no launch shape and no order among equal values enters a
 *            result, and results compare bit for bit with a sequential evaluation. */
#define EPI_PADJ_NONE        0
#define EPI_PADJ_BONFERRONI  1
#define EPI_PADJ_HOLM        2
#define EPI_PADJ_HOCHBERG    3
#define EPI_PADJ_BH          4
#define EPI_PADJ_BY          5
int epi_p_adjust_dev(epi_engine *e, const double *d_p, int64_t n, int32_t method, int64_t n_tests, double *d_q,
                     int32_t *d_order, void *stream, int64_t *nvalid_out);

/* Tail probabilities of the chi-square, Student and F(1, df) distributions.  The reference has no such call.  One copy of
 * the arithmetic (csrc/dist_math.hpp, which has the formulas) is compiled into the host function and the device kernel,
 * without fast-math and without contraction.
 *  Kinds     EPI_DIST_CHISQ  p = P(X >= x), X chi-square with df degrees of freedom: Q(df / 2, x / 2), the regularised upper
 *                            incomplete gamma function (series below x / 2 < df / 2 + 1, continued fraction above it,
 *                            erfc(sqrt(x / 2)) at df == 1).
 *            EPI_DIST_T2     x is a Student statistic t, of either sign; p = P(|T| >= |t|) = I_{df / (df + t^2)}(df / 2, 1 / 2),
 *                            the regularised incomplete beta function (continued fraction with the symmetric swap).
 *            EPI_DIST_F1     x is an F statistic with 1 and df degrees of freedom; p = P(F >= x) = I_{df / (df + x)}(df / 2, 1 / 2).
 *  Domain    df finite, 0 < df <= 1e4.  x >= 0 (EPI_DIST_T2: any t).  x == 0 gives 1, +inf (EPI_DIST_T2: either inf) gives
 *            0.  NaN, a negative x, or a df outside the range: NaN.  No loop depends on convergence alone: each has a fixed
 *            bound derived from the domain, and a tail that has not converged there is NaN (none does on the domain).
 *  Accuracy  against 50-digit arithmetic on the grid and the random points of tests/test_dist_host.py the host's largest
 *            relative error is 6.4e-13 where the exact value is at least 1e-300 (EPI_DIST_T2 at t = 2, df = 1e4, just below the
 *            swap, where the direct fraction's denominators cancel; the chi-square tail's is 1.1e-13, at p = 4e-249, about
 *            1e-16 times the size of the exponent); below 1e-300 the result is between 0 and 1e-300.  The device differs from the host by
 *            what its lgamma / log / exp / erfc differ (DESIGN 4.18 has the measured figure).
 * epi_dist_tail is host code and needs no device.  epi_dist_tail_dev: all pointers are device memory of e's device, one
 * thread per value performs the host's operations in the host's order, so no launch shape enters a result; the kernel is
 * queued on `stream`, nothing is synchronised.  n == 0: nothing is done.  A kind other than the three, n < 0 or a NULL
 * pointer with n > 0: EPI_ERR_ARG. */
#define EPI_DIST_CHISQ 0
#define EPI_DIST_T2    1
#define EPI_DIST_F1    2
int epi_dist_tail(int32_t kind, const double *x, const double *df, int64_t n, double *p_out);
int epi_dist_tail_dev(epi_engine *e, int32_t kind, const double *d_x, const double *d_df, int64_t n, double *d_p, void *stream);

/* Two groups of cytosine reports against each other per cytosine: replicate-aware differential methylation.  The reference
 * has no such report.  Stateless, like epi_cx_compare_dev: the call reads device columns of the caller, writes device columns
 * of the caller, holds its scratch for the length of the call (epi_device_allocations reads the same after it as before,
 * on every return path) and touches no batch.  It synchronises `stream`, once before anything is written.
 *  Inputs    d_tabs: (n_a + n_b) * 6 device pointers (the array itself is host memory), the six CX columns (rname, strand, pos,
 *            context, meth, unmeth) of each sample, group a's samples first; nrows[k]: the rows of sample k.  n_a and n_b from
 *            1 to 32, the rows of all samples together below 2^32.  Precondition, checked on the device: the rows of every
 *            table strictly ascend in (rname, pos, strand); otherwise EPI_ERR_ARG naming a table, and nothing is written.
 *  Key       one 64-bit key per row: rname << 35 | pos << 4 | (strand - 1) << 3 | context.  rname codes from 0 to
 *            EPI_CXG_MAX_RNAME = 2^21 - 1, pos from 0 to 2^31 - 1, strand 1 or 2, context codes from 0 to 7, meth and unmeth not
 *            negative: anything else in any row is EPI_ERR_ARG, and nothing is written.
 *  Sites     a site is a distinct (rname, pos, strand, context) over all tables.  Sample k counts at a site when it has that
 *            row with meth + unmeth >= max(min_coverage, 1).  *nsite_out = the sites at which at least one sample counts.  A
 *            site is reported when at least min_samples_a samples of a and min_samples_b samples of b count (each minimum
 *            from 1 to its group's size, else EPI_ERR_ARG), in ascending (rname, pos, strand, context).  *nrow_out = their
 *            number.
 *  Columns   ten int32: rname, strand, pos, context, meth_a, unmeth_a, meth_b, unmeth_b (M_g, U_g: sums over the counting
 *            samples of the group), nsamples_a, nsamples_b (n_a', n_b': the counting samples).  If N_g = M_g + U_g of a reported
 *            site exceeds 2^31 - 1: EPI_ERR_ARG, nothing is written.  Eleven double: beta_a = M_a / N_a, beta_b (one IEEE
 *            division of integers each), delta_beta = beta_b - beta_a; mean_beta_g = (sum in sample order of beta_i = m_i /
 *            (m_i + u_i)) / n_g'; var_g = (sum in sample order of (beta_i - mean_beta_g)^2) / (n_g' - 1), NaN when n_g' < 2;
 *            stat, df, phi, p by `test`:
 *  Tests     with p0 = (M_a + M_b) / (N_a + N_b), q0 = (U_a + U_b) / (N_a + N_b), n = n_a' + n_b', d(x, e) = e when x == 0 and
 *            else csrc/fisher_math.hpp's deviance term bd0(x, e) = x log(x / e) + e - x,
 *            G = 2 (((d(M_a, N_a p0) + d(U_a, N_a q0)) + d(M_b, N_b p0)) + d(U_b, N_b q0)), every term >= 0:
 *              EPI_CXG_FISHER  p = the two-sided Fisher p-value of (M_a U_a / M_b U_b) as epi_fisher_exact_dev computes it;
 *                              stat, df, phi NaN.  With one sample a side the table is epi_cx_compare_dev's.
 *              EPI_CXG_LRT     the likelihood-ratio test of the two-group binomial logistic regression: stat = G, df = 1, phi
 *                              NaN, p = EPI_DIST_CHISQ of (G, 1).  M = 0 or U = 0 in both groups: G = 0 and p = 1 exactly.
 *              EPI_CXG_LRT_MN  the same deviance with McCullagh-Nelder overdispersion and an F test: X2 = the sum, over a's
 *                              counting samples and then b's, in sample order, of (m_i - n_i ph_g)^2 / ((n_i ph_g) (1 - ph_g))
 *                              with n_i = m_i + u_i, ph_g = M_g / N_g, a term with a zero denominator being 0; phi = max(1, X2 /
 *                              (n - 2)), stat = G / phi, df = n - 2, p = EPI_DIST_F1 of (stat, df).  n <= 2: df = n - 2 and
 *                              stat, phi, p NaN.
 *              EPI_CXG_WELCH   Welch's t-test on the samples' betas: v_g = var_g / n_g', s2 = v_a + v_b, stat = (mean_beta_b -
 *                              mean_beta_a) / sqrt(s2), df = s2^2 / (v_a^2 / (n_a' - 1) + v_b^2 / (n_b' - 1)), p = EPI_DIST_T2 of
 *                              (stat, df); phi NaN.  n_a' < 2, n_b' < 2 or s2 == 0: stat, df, p NaN.
 *            One thread per reported site performs these operations in this order: no launch shape enters a result, and the
 *            integer columns, the betas, means, variances, phi and Welch's stat and df compare bit for bit with a sequential
 *            evaluation in IEEE double; G and p differ by what the device's log / exp / lgamma / erfc differ from the host's.
 *  Capacity  the columns hold `cap` rows.  cap < *nrow_out: EPI_ERR_ARG, nothing is written, *nrow_out is the count needed.
 *            (rows of all samples) / (min_samples_a + min_samples_b) always suffices.  No rows at all: an empty report.
 *  Memory    32 bytes per input row (two key and two value buffers of the sort, the rows' two counts) and the sort's digit
 *            tables; epi_cx_groups_scratch_bytes gives the figure for total_rows rows, 0 for none, or EPI_ERR_ARG outside
 *            0 <= total_rows < 2^32 (it needs no device).
 * No covariates, no beta-binomial shrinkage, no sharded form. */
#define EPI_CXG_FISHER 0
#define EPI_CXG_LRT    1
#define EPI_CXG_LRT_MN 2
#define EPI_CXG_WELCH  3
#define EPI_CXG_MAX_RNAME 2097151
int epi_cx_groups_dev(epi_engine *e, const int32_t *const *d_tabs, const int64_t *nrows, int32_t n_a, int32_t n_b,
                      int32_t min_coverage, int32_t min_samples_a, int32_t min_samples_b, int32_t test,
                      int32_t *const d_icols[10], double *const d_dcols[11], int64_t cap, void *stream, int64_t *nsite_out,
                      int64_t *nrow_out);
int epi_cx_groups_scratch_bytes(int64_t total_rows, int64_t *bytes_out);

/* CpG strand merging of a cytosine report (Bismark --merge_CpG, methylKit destrand = TRUE): the '-' row of a CpG at pos + 1 is
 * added to the '+' row at pos.  The reference has no such call.  Stateless, like epi_cx_compare_dev: the call reads the six
 * device columns of a CX table (rname, strand, pos, context, meth, unmeth), writes six device columns of the caller (which must
 * not overlap the input), holds its scratch (8 bytes per row) for the length of the call (epi_device_allocations reads the
 * same after it as before, on every return path) and touches no batch.  It synchronises `stream`, once before anything is
 * written.
 *  Input     precondition, checked on the device: the rows strictly ascend in (rname, pos, strand), strand is 1 or 2, meth
 *            and unmeth are not negative.  Otherwise EPI_ERR_ARG, and nothing is written.
 *  Minus CpG a row with strand 2 whose context code is 7 (CG).  Its partner: the row immediately before it, when that has the
 *            same rname, pos one less, strand 1 and context code 7.
 *  Rows      a minus CpG (rname, q, '-') with a partner: ONE output row at the partner's place -- the partner's rname, strand
 *            1, the partner's pos, context 7, meth and unmeth summed; a sum above 2^31 - 1 is EPI_ERR_ARG, and nothing is
 *            written.  Without a partner: the row becomes (rname, 1, q - 1) with its own context and counts when q >= 2 and
 *            the row before it, if any, is strictly below (rname, q - 1, '+') in table order; otherwise it is left exactly as
 *            it is (something already stands at or above (rname, q - 1, '+'): a non-CG '+' row there, or a '-' row).  Every
 *            other row is copied unchanged.  The output strictly ascends again: a moved row stays above its predecessor by
 *            the rule that lets it move, and below its successor, which was above (rname, q, '-').
 *  Counts    *nrow_out = the output's rows = n - *nmerged_out; *nmerged_out = the pairs; *nmoved_out = the minus CpGs that
 *            moved; *nkept_out = the minus CpGs left as they are.
 *  Capacity  the columns hold `cap` rows.  cap < *nrow_out: EPI_ERR_ARG, nothing is written, *nrow_out is the count needed.
 *            cap >= n always suffices.  n == 0: an empty table.  n >= 2^31: EPI_ERR_ARG. */
int epi_cx_merge_strands_dev(epi_engine *e, const int32_t *const d_in[6], int64_t n, int32_t *const d_out[6], int64_t cap,
                             void *stream, int64_t *nrow_out, int64_t *nmerged_out, int64_t *nmoved_out, int64_t *nkept_out);

/* Local-regression smoothing of a cytosine report (the idea of bsseq's BSmooth and DSS's smoothing): a tricube-weighted,
 * coverage-weighted local polynomial of methylation over neighbouring cytosines, with a bandwidth that widens where
 * cytosines are sparse.  The reference has no such call.  Stateless, like epi_cx_compare_dev: six device columns of a CX
 * table in (thresholded or not, merged or not), nine int32 and three double device columns of n rows each out, in the
 * input's row order (they must not overlap the input); the scratch is held for the length of the call
 * (epi_device_allocations reads the same after it as before, on every return path), no batch is touched.  It synchronises
 * `stream`, once before anything is written.
 *  Input     precondition, checked on the device: the rows strictly ascend in (rname, pos, strand); strand is 1 or 2; the
 *            context code is 0 to 7; pos, meth and unmeth are not negative.  Otherwise EPI_ERR_ARG, nothing is written.
 *  Limits    degree 0 to EPI_SMOOTH_MAX_DEGREE, bandwidth 1 to EPI_SMOOTH_MAX_BANDWIDTH, max_gap >= 0, min_sites 1 to
 *            EPI_SMOOTH_MAX_WINDOW, 0 <= n < 2^31: anything else is EPI_ERR_ARG before any device work.
 *  Series    the rows of one (rname, strand, context code), in ascending pos.  Every row is smoothed within its own series:
 *            both strands and several contexts may be interleaved.  A series is cut into clusters wherever two neighbours
 *            are MORE than max_gap apart.  *ncluster_out = the clusters.
 *  Window    site i of a cluster of c sites: k = min(min_sites, c); D_i = the smallest distance within which at least k
 *            sites of the cluster lie, site i included (the k-th smallest |pos_j - pos_i|); H_i = max(bandwidth, D_i).  The
 *            window's sites are those of the cluster with |pos_j - pos_i| < H_i (a site at exactly H_i has weight 0).
 *            *max_window_out = the largest number of sites in a window.  Above EPI_SMOOTH_MAX_WINDOW: EPI_ERR_ARG, found
 *            before any fit runs, nothing is written -- a careless bandwidth does not become an n^2 kernel.
 *  Fit       all in fp64, every product and sum one correctly rounded operation, in exactly this order (one copy of it,
 *            csrc/smooth_math.hpp, is compiled into the host function and the kernel without fast-math and without
 *            contraction).  Per window site j in ascending j, accumulated by the one thread that owns site i:
 *              d = pos_j - pos_i (integer)   u = (double)d / (double)H_i   a = |u|
 *              c = 1 - (a*a)*a               t = (c*c)*c                   u2 = u*u
 *              w = t * (double)(meth_j + unmeth_j)                         v = t * (double)meth_j
 *              S0 += w   S1 += w*u   S2 += w*u2   S3 += (w*u2)*u   S4 += (w*u2)*u2
 *              T0 += v   T1 += v*u   T2 += v*u2
 *            The intercept at u = 0 by an LDL^T solve of the weighted normal equations, a relative pivot test lowering the
 *            degree (kPivot = 1e-4):
 *              not (S0 > 0)                                   -> smoothed = NaN, degree_used = -1
 *              d0 = S0; l10 = S1/d0; d1 = S2 - l10*S1
 *              degree >= 1 and d1 > kPivot*S2                 -> degree_used >= 1, else 0
 *              l20 = S2/d0; l21 = (S3 - l20*S1)/d1; d2 = (S4 - l20*S2) - l21*(l21*d1)
 *              degree == 2 and d2 > kPivot*S4                 -> degree_used = 2
 *              deg 0: a0 = T0/d0
 *              deg 1: z1 = T1 - l10*T0;  a1 = z1/d1;  a0 = T0/d0 - l10*a1
 *              deg 2: z1 as above;  z2 = (T2 - l20*T0) - l21*z1;  a2 = z2/d2;  a1 = z1/d1 - l21*a2
 *                     a0 = (T0/d0 - l10*a1) - l20*a2
 *              smoothed = min(1, max(0, a0))
 *            No launch shape enters a result: the columns compare bit for bit with a sequential evaluation in IEEE double.
 *            Against exact rational arithmetic with the fit of the same degree_used the largest absolute error of smoothed
 *            is 1.8e-12 (tests/test_smooth_host.py; the pivot test is what keeps one-sided windows at cluster ends from
 *            extrapolating through nearly collinear points).
 *  Columns   nine int32: the six of the input, nsites = the window's sites at any coverage, halfwidth = H_i, degree =
 *            degree_used.  Three double: beta = meth / (meth + unmeth), one IEEE division, NaN at zero coverage; smoothed;
 *            weight = S0.  A site with zero coverage still gets a smoothed value from its neighbours.
 *  Memory    52 bytes per row (the sort's workspace, 24; pos, meth, coverage in series order, H, window bounds and cluster
 *            starts, 28) and the sort's digit tables; epi_cx_smooth_scratch_bytes gives the figure for n rows, 0 for none,
 *            or EPI_ERR_ARG outside 0 <= n < 2^31 (it needs no device).
 * epi_smooth_window is host code and needs no device: the same arithmetic over the window of site i of ONE series (pos
 * ascending, n >= 1 sites, 0 <= i < n, halfwidth >= 1 given by the caller): the sites with |pos_j - pos_i| < halfwidth in
 * ascending j; *weight = S0.  epi_smooth_tile_sites and epi_smooth_stage_sites: the consecutive series-ordered sites a
 * workgroup of the fit kernel owns, and the largest range of sites it stages in LDS (a longer one is read from global
 * memory, with the same results).
 * No binomial local likelihood, no standard errors, no sharded form. */
#define EPI_SMOOTH_MAX_DEGREE 2
#define EPI_SMOOTH_MAX_BANDWIDTH 1073741824
#define EPI_SMOOTH_MAX_WINDOW 65536
int epi_cx_smooth_dev(epi_engine *e, const int32_t *const d_in[6], int64_t n, int32_t bandwidth, int32_t min_sites,
                      int32_t max_gap, int32_t degree, int32_t *const d_icols[9], double *const d_dcols[3], void *stream,
                      int64_t *ncluster_out, int64_t *max_window_out);
int epi_cx_smooth_scratch_bytes(int64_t n, int64_t *bytes_out);
int epi_smooth_window(const int32_t *pos, const int32_t *meth, const int32_t *unmeth, int64_t n, int64_t i, int32_t halfwidth,
                      int32_t degree, double *smoothed, int32_t *degree_used, double *weight);
int epi_smooth_tile_sites(void);
int epi_smooth_stage_sites(void);

/* Methylation segments of ONE sample's cytosine report: a small hidden Markov model over the series of cytosines, decoded by
 * exact Viterbi and refitted by hard EM (the idea of MethylSeekR's UMR / LMR / PMD and of methpipe's hmr / pmd).  The
 * reference has no such call.  Stateless, like epi_cx_smooth_dev: six device columns of a CX table in; one int32 device
 * column of n states out, in the input's row order, and a segment table of seven int32 and three double device columns (none
 * may overlap the input); the scratch is held for the length of the call (epi_device_allocations reads the same after it as
 * before, on every return path), no batch is touched.  It synchronises `stream`: once for the input's verdict, once per refit
 * iteration, and once before anything is written.  The whole model is stated in integers, so the parallel decode equals the
 * sequential loop at every tie: no result depends on a launch shape and nothing is compared with a tolerance.
 *  Input     precondition, checked on the device, the smoother's: the rows strictly ascend in (rname, pos, strand); strand
 *            is 1 or 2; the context code is 0 to 7; pos, meth and unmeth are not negative.
 *  Series    the smoother's order and cuts: the rows ordered by class (strand - 1) * 8 + context, stably, so a class ascends
 *            in (rname, pos).  A CHAIN starts at a class change, at an rname change, or where pos - previous pos > max_gap.
 *            *nchain_out = the chains.
 *  Model     K = nstates states, EPI_SEGMENT_MIN_STATES <= K <= EPI_SEGMENT_MAX_STATES.  p[k]: the methylation level of state
 *            k; trans[j * K + k]: the transition from j to k; init[k]: the initial distribution.  Every entry of all three
 *            lies in [2^-16, 1] (p additionally <= 1 - 2^-16); every row of trans, and init, sums to 1 within 1e-9 (summed
 *            in index order).  States need not be ordered or distinct.
 *  Quantise  q(x) = floor(log(x) * 65536 + 0.5) as an integer; log is libm's in fp64, in a host unit built without fast-math
 *            and without contraction.  A[k] = q(p[k]), B[k] = q(1 - p[k]), T[j][k] = q(trans[j][k]), I[k] = q(init[k]): all
 *            <= 0, and >= -726817 for a caller's parameters.
 *  Counts    cov = meth + unmeth in int64; if cov > max_coverage then m' = (meth * max_coverage) / cov (integer division)
 *            and u' = max_coverage - m', else m' = meth, u' = unmeth.  1 <= max_coverage <= EPI_SEGMENT_MAX_COVERAGE.
 *            The emission of site i in state k is e_i(k) = m'_i * A[k] + u'_i * B[k] in int64 (the binomial coefficient is
 *            the same for every state and is left out).
 *  Decode    per chain of sites 0 .. L - 1:  delta_0(k) = I[k] + e_0(k);  delta_i(k) = max_j (delta_{i-1}(j) + T[j][k]) +
 *            e_i(k), psi_i(k) = the SMALLEST j attaining that maximum; the last state is the SMALLEST k attaining max
 *            delta_{L-1}; state_{i-1} = psi_i(state_i).  The chain's score is max delta_{L-1}; score = the sum of the chains'
 *            scores.
 *  Bound     n <= EPI_SEGMENT_MAX_SITES = 2^26.  A site adds at least -(32767 * 726817 + 2^21) > -2^35 to a score (a
 *            refitted transition or start is >= q(1 / (2^26 + 4)) = -1181078 > -2^21), so every partial score lies in
 *            (-2^62, 0]: nothing can overflow.
 *  Refit     hard EM, max_iter >= 1 decodes.  For it = 1 .. max_iter: decode; if it == max_iter stop.  Count over all chains
 *            in int64: M[k], U[k] = the sums of m', u' over the sites in state k; N[j][k] = adjacent in-chain pairs going
 *            from j to k; S[k] = chains that start in state k.  Re-estimate on the host in fp64, one IEEE division each:
 *            p[k] = (M + 1) / (M + U + 2), clamped to [2^-16, 1 - 2^-16], kept when M + U = 0; trans[j][k] = (N[j][k] + 1) /
 *            (sum_k N[j][k] + K), the row kept when its sum is 0; init[k] = (S[k] + 1) / (sum S + K).  Quantise; if all four
 *            tables equal the previous iteration's, converged = 1 and stop.  The parameters reported are those of the last
 *            decode; iterations = the decodes.  max_iter = 1 is a pure decode with the caller's parameters.
 *  Outputs   d_state[row] = the row's state.  The segment table: the maximal runs of one state inside a chain, in series
 *            order; int32 rname, strand, context, start, end (the first and last site's pos), state, nsites; double meth,
 *            unmeth (the run's RAW counts, summed in int64 and converted: exact, they are below 2^53) and beta = meth /
 *            (meth + unmeth), NaN at 0 / 0.  *nsegment_out = its rows; *fit_out = the fit.
 *  Errors    EPI_ERR_ARG for anything outside the above (n > 2^26 is refused before any pointer is read).  On any error
 *            nothing is written, neither columns nor outputs -- but when the segment table needs more than seg_cap rows,
 *            *nsegment_out is set to the count needed (the message names "rows to write, room for").  seg_cap >= n always
 *            suffices.  n == 0: EPI_OK, iterations = 0, score = 0, the caller's parameters in *fit_out, no column touched.
 *  Memory    about 30 bytes per row (the sort's workspace, 24; a word, an f byte and a state per site) plus 8 K^2 + 8 K + 10
 *            bytes per epi_segment_block_sites() rows; epi_cx_segment_scratch_bytes gives the figure, 0 for no rows, or
 *            EPI_ERR_ARG outside 0 <= n <= 2^26 or for a bad nstates (it needs no device).
 * Host functions that need no device (csrc/segment_host.cpp, on the arithmetic the kernels share, csrc/segment_math.hpp):
 * epi_segment_quantise: the argument checks of Model, then tables_out = A[K], B[K], T[K * K] (row-major), I[K].
 * epi_segment_reestimate: the re-estimate of Refit, in place, from counts = M[K], U[K], N[K * K], S[K] (each 0 to 2^42).
 * epi_segment_chain_host: the plain loop of Decode over ONE chain of 1 <= n <= 2^26 sites from such tables (A and B in
 * [-726817, 0], T and I in [-2^21, 0]): n states and the chain's score.
 * epi_segment_block_sites, epi_segment_thread_sites: the series-ordered sites one workgroup scans and one thread walks.
 * No posterior probabilities (forward-backward), no distance-dependent transitions, no beta-binomial emissions, no sharded form. */
#define EPI_SEGMENT_MIN_STATES 2
#define EPI_SEGMENT_MAX_STATES 4
#define EPI_SEGMENT_MAX_COVERAGE 32767
#define EPI_SEGMENT_MAX_SITES 67108864
typedef struct {
  int32_t nstates, iterations, converged, unused;
  int64_t score;
  double p[4], trans[16], init[4];          /* trans: nstates x nstates, row-major, packed */
} epi_segment_fit;
int epi_cx_segment_dev(epi_engine *e, const int32_t *const d_in[6], int64_t n, int32_t nstates, const double *p,
                       const double *trans, const double *init, int32_t max_gap, int32_t max_coverage, int32_t max_iter,
                       int32_t *d_state, int32_t *const d_seg_i[7], double *const d_seg_d[3], int64_t seg_cap, void *stream,
                       epi_segment_fit *fit_out, int64_t *nchain_out, int64_t *nsegment_out);
int epi_cx_segment_scratch_bytes(int64_t n, int32_t nstates, int64_t *bytes_out);
int epi_segment_quantise(int32_t nstates, const double *p, const double *trans, const double *init, int32_t *tables_out);
int epi_segment_reestimate(int32_t nstates, const int64_t *counts, double *p, double *trans, double *init);
int epi_segment_chain_host(int32_t nstates, const int32_t *tables, const int32_t *meth, const int32_t *unmeth, int64_t n,
                           int32_t max_coverage, int32_t *state_out, int64_t *score_out);
int epi_segment_block_sites(void);
int epi_segment_thread_sites(void);

/* rcpp_extract_patterns (src/rcpp_extract_patterns.cpp:26-211; caller .getPatterns, R/internal.R:683-714):
 * methylation patterns of the reads overlapping one target.  Library-owned host table: per pattern strand, start,
 * end, nbase, beta, the FNV-1a hash the R side prints as 16 hex digits ("pattern"), the ordered column positions
 * and cells[col * npat + p] = context index / base factor code (levels as :192-195) or INT32_MIN (NA).
 * npat = 0 is the reference's empty data frame.  One target against all rows of the batch: device scratch of 8 B per row
 * (allocated and freed by the call), the two passes and the host round trips of epi_batch_extract_patterns_multi below.
 * Leaves that call's statistics alone.  Synchronises `stream`. */
typedef struct {
  int64_t npat;
  int32_t ncol;
  int32_t *positions;                       /* [ncol] */
  int32_t *strand, *start, *end, *nbase;    /* [npat] */
  double *beta;                             /* [npat] */
  uint64_t *fnv;                            /* [npat] */
  int32_t *cells;                           /* [ncol][npat] */
} epi_pattern_table;
int epi_batch_extract_patterns(epi_batch *b, int32_t target_rname, int32_t target_start, int32_t target_end,
                               int32_t min_overlap, const char *ctx, double min_ctx_freq, int32_t clip,
                               int32_t reverse_offset, const int32_t *hlght /* sorted, unique, inside the target */,
                               int32_t nhlght, void *stream, epi_pattern_table *out);
void epi_pattern_table_free(epi_pattern_table *t);
/* The same for every target of a list in one pass: out[t] is what epi_batch_extract_patterns returns for
 * (target_rname[t], target_start[t], target_end[t]) with the highlight positions hlght[hlght_off[t] .. hlght_off[t+1])
 * (each slice sorted, unique, inside its target; hlght_off NULL = none) and the same other arguments; targets may
 * overlap, repeat and come in any order.  Each out[t] is released with epi_pattern_table_free; on any failure every
 * out[t] is left zeroed and freed.  ntargets == 0 and an empty batch return EPI_OK.
 * Row order: the rows must be sorted by (rname, start), as preprocessBam leaves them.  The candidate rows of a target
 * -- its rname, start in [start - Lmax + 1, end], Lmax the longest row -- are then one row range found by search, and
 * the work is one flat list of (target, candidate row) pairs: cost O(candidate rows), a fixed number of launches and
 * three host synchronisations per GROUP of targets, whatever their number.  For rows in another order (adopted
 * columns), rows or targets with negative coordinates, the call runs target by target instead, every target against all
 * rows as epi_batch_extract_patterns does, with one scratch for the list: same tables, cost O(rows x targets), 8 B of
 * scratch per row of the batch.
 * Memory: nothing is sized by the batch.  Consecutive targets form a group while 40 B per pair + 8 B per window position
 * (end - start + 2 Lmax + reverse_offset + 8 per target) stay under a cap of 256 MiB; the results of a group (32 B per
 * overlapping row + 4 B per cell) are fetched in batches under the same cap.  A target above the cap runs alone.
 * Device scratch (allocated and freed by the call, buffers grown with 1/8 of slack) is therefore at most 600 MiB + 200 B
 * per target unless one target exceeds the cap by itself; the host holds the same plus the tables.  Synchronises `stream`. */
int epi_batch_extract_patterns_multi(epi_batch *b, int32_t ntargets, const int32_t *target_rname,
                                     const int32_t *target_start, const int32_t *target_end, int32_t min_overlap,
                                     const char *ctx, double min_ctx_freq, int32_t clip, int32_t reverse_offset,
                                     const int32_t *hlght, const int64_t *hlght_off /* [ntargets+1] CSR, may be NULL */,
                                     void *stream, epi_pattern_table *out /* [ntargets] */);
/* Of the last epi_batch_extract_patterns_multi on this batch: groups run (0: the target-by-target path), (target,
 * candidate row) pairs, peak device scratch in bytes.  Any pointer may be NULL. */
int epi_batch_extract_patterns_multi_stats(epi_batch *b, int64_t *groups, int64_t *pairs, int64_t *scratch_bytes);

/* The unique patterns of every target with their counts: what plotPatterns makes of extractPatterns' table before it
 * draws, patterns[, .(count=.N), by=c("pattern", base.positions)] (R/plotPatterns.R:170-172).  With P the table
 * epi_batch_extract_patterns returns for target t and the same arguments, out[t] holds the unique rows of P by (fnv, every
 * cell) in the order of their first appearance in P: fnv, count, cells[col * nuniq + u]; npat = P's rows = the sum of the
 * counts.  Strand, start, end and nbase are not part of the key and are not returned.  Library-owned, released with
 * epi_pattern_summary_free; on any failure every out[t] is left zeroed and freed.  nuniq = 0: P is empty.
 * The rows are grouped on the device, behind the second pass of epi_batch_extract_patterns_multi (same arguments, same
 * groups of targets): one open-addressing table per batch of results, every target a slice of a power-of-two capacity
 * >= 2 x its overlapping rows, keyed by the hash; a wave adds once per distinct key among its lanes.  Every row is then
 * compared, cell by cell, with the first row of its table entry.  A target in which two different patterns met under one
 * key is grouped on the host instead, by (fnv, cells), from its per-row results: the result never rests on the hash.
 * So are the targets of the target-by-target path (rows in another order, negative coordinates), from their tables.
 * Transfer: 12 B + 4 B per column for every UNIQUE pattern, plus 12 B per target; nothing per row.
 * Memory: as epi_batch_extract_patterns_multi, and inside the same cap: a batch of results counts 16 B per table entry
 * (at most 4 x the overlapping rows + 8 per target), 20 B per overlapping row and its unique rows at their most (12 B per
 * overlapping row + 4 B per cell) on top of that call's 32 B per overlapping row + 4 B per cell.  The device indexes slots,
 * cells and table entries with 32 bits: a batch of results with 2^30 overlapping rows, 2^31 cells or 2^32 table entries or
 * more (one target far above the cap) is grouped on the host, its targets counted as such.  Synchronises `stream`. */
typedef struct {
  int64_t nuniq, npat;
  int32_t ncol;
  int32_t *positions;                       /* [ncol] */
  uint64_t *fnv;                            /* [nuniq] */
  int32_t *count;                           /* [nuniq] */
  int32_t *cells;                           /* [ncol][nuniq] */
} epi_pattern_summary;
void epi_pattern_summary_free(epi_pattern_summary *t);
int epi_batch_summarise_patterns_multi(epi_batch *b, int32_t ntargets, const int32_t *target_rname,
                                       const int32_t *target_start, const int32_t *target_end, int32_t min_overlap,
                                       const char *ctx, double min_ctx_freq, int32_t clip, int32_t reverse_offset,
                                       const int32_t *hlght, const int64_t *hlght_off /* [ntargets+1] CSR, may be NULL */,
                                       void *stream, epi_pattern_summary *out /* [ntargets] */);
/* Of the last epi_batch_summarise_patterns_multi on this batch: groups run (0: the target-by-target path), (target,
 * candidate row) pairs, targets that were grouped on the host.  Any pointer may be NULL. */
int epi_batch_summarise_patterns_stats(epi_batch *b, int64_t *groups, int64_t *pairs, int64_t *fallback_targets);

/* rcpp_get_base_freqs on a resident batch (see epi_get_base_freqs): d_site_chr / d_site_pos are nsite device int32
 * (rname codes, 1-based positions) sorted by (code, pos), NA-coded sites removed -- equal keys (multi-ALT records) are
 * allowed; EPI_ERR_UNSORTED otherwise, or when the rows are not sorted by (rname, start).  d_counts [20][nsite] u32 is
 * overwritten (column-major as the drop-in's matrix).  d_pass: per-row flags or NULL = all TRUE.  Reads the rows through
 * the batch's own view (every row layout).  Synchronises `stream` once (the two sortedness verdicts), then queues the
 * counting kernel.  The counts are additive over row shards. */
int epi_batch_base_freqs_dev(epi_batch *b, const int32_t *d_pass /* NULL = all TRUE */, const int32_t *d_site_chr,
                             const int32_t *d_site_pos, int64_t nsite, uint32_t *d_counts /* [20][nsite] */, void *stream);

/* ---- multi-GPU (row-range shards; see DESIGN.md "Multi-GPU") -------------
 * Tiles are cut on an absolute position grid (epi_tile_positions() wide), so
 * ranks agree on tile boundaries.  A rank (a) reports the range of tile keys
 * its rows touch, (b) is told which keys are shared with other ranks; shared
 * tiles are accumulated into a dense counter slab instead of being emitted,
 * (c) the caller sum-reduces the slabs across ranks (RCCL all-reduce), and
 * (d) the owning rank emits them.  key = ((int64)rname << 32) | biased tile.  Slab planes of one tile: (n, M) per
 * strand and reported context, then the two strands' coverage difference arrays (cx_report.hip). */
int epi_tile_positions(void);                  /* CX tile size for a single-context report (e.g. "Z") */
int epi_cx_tile_positions(const char *ctx);    /* ... for this context string: 2048 with one reported context, else 1024 */
int epi_batch_tile_key_range(epi_batch *b, void *stream, int64_t *first_key, int64_t *last_key);
int epi_batch_cx_set_shared(epi_batch *b, const int64_t *h_keys, const int32_t *h_owned,
                            int32_t nshared, int32_t *d_slab /* [nshared][16][T] int32, zeroed by caller */);
/* With shared tiles set, epi_batch_cx_report_dev stops after accumulation
 * (nrow_out = 0); all-reduce the slab, then finish: */
int epi_batch_cx_finish_shared(epi_batch *b, const char *ctx, void *stream, int64_t *nrow_out);

/* The same exchange for the lMHL table (tiles of epi_mhl_tile_positions() positions): shared tiles
 * hand over their counters [nshared][16][T] (int32) and their numerator sums / interval arrays
 * [nshared][epi_mhl_slab_sums()] (int64, wrap-around arithmetic); all-reduce both, then finish. */
int epi_mhl_tile_positions(void);
int epi_mhl_slab_sums(void);
int epi_batch_tile_key_range_for(epi_batch *b, int tile_positions, void *stream, int64_t *first_key, int64_t *last_key);
int epi_batch_mhl_set_shared(epi_batch *b, const int64_t *h_keys, const int32_t *h_owned, int32_t nshared,
                             int32_t *d_cnt_slab, int64_t *d_sum_slab);
int epi_batch_mhl_finish_shared(epi_batch *b, void *stream, int64_t *nrow_out);
/* The one-pass lMHL kernel shards as well: tiles of epi_mhl_fused_tile_positions() positions, slabs int32
 * [nshared][4][T] (calls of the context '+', '-'; coverage differences '+', '-') and int64 [nshared][6][T] (difference
 * arrays of the three sums, two strands each).  Every rank must take the same path: epi_batch_mhl_fused_ok says whether
 * THIS rank's rows allow the one-pass kernel for `ctx` (one haplotype context, reads of at most 4 KiB); the caller
 * combines the answers (distributed.py: all ranks, once per shard) and attaches the slabs with the matching call.
 * epi_batch_mhl_report_dev and epi_batch_mhl_finish_shared are then used as for the two-kernel layout. */
int epi_mhl_fused_tile_positions(void);
int epi_batch_mhl_fused_ok(epi_batch *b, const char *ctx, void *stream, int32_t *ok_out);
int epi_batch_mhl_set_shared_fused(epi_batch *b, const int64_t *h_keys, const int32_t *h_owned, int32_t nshared,
                                   int32_t *d_cnt_slab, int64_t *d_sum_slab);

/* ---- the same exchange with RCCL called by the library (csrc/comm.hip) -------------------------------------------
 * For hosts without a collective library of their own (the R shim): one epi_comm per process
 * and GPU, one call per report.  The 128-byte id comes from ONE rank (epi_comm_unique_id = ncclGetUniqueId) and travels
 * to the others by whatever the host has; epi_comm_create is collective (ncclCommInitRank).  Every rank then calls the
 * sharded entry point on its own batch -- a contiguous range of the globally (rname, start)-sorted rows, ranges in rank
 * order: tile key ranges are all-gathered (once per batch and tile grid), shared tiles accumulate into a slab owned by
 * the batch, ncclAllReduce runs on the report's stream, owners emit.  nrow_out = THIS rank's rows; the reference's table
 * is the ranks' tables in rank order (epi_batch_cx_fetch_* / epi_batch_mhl_fetch_* as after a single-GPU report).
 * Replaces, for the sharded path, R/generateCytosineReport.R:181-203 and R/generateMhlReport.R:185-196 run on the whole
 * data set.  ctx_meth == NULL: no thresholding (d_pass: per-row flags in device memory or NULL = all TRUE). */
/* Step 2 on its own (pure host logic, no device needed): ranges = (first, last) tile key per rank, first > last for a rank
 * without rows; keys_out / owner_out (capacity cap; cap = 0: only count) receive the keys reachable from at least two ranks,
 * ascending, and the lowest rank that reaches each.  What epialleler_amd/distributed.py's shared_tile_keys computes. */
int epi_shared_tile_keys(const int64_t *ranges, int32_t world, int64_t *keys_out, int32_t *owner_out, int32_t cap, int32_t *n_out);
#define EPI_COMM_ID_BYTES 128
typedef struct epi_comm epi_comm;
int epi_comm_unique_id(void *id_out /* EPI_COMM_ID_BYTES */);
int epi_comm_create(epi_engine *eng, const void *id /* EPI_COMM_ID_BYTES; may be NULL when world == 1 */, int rank, int world,
                    epi_comm **out);
void epi_comm_free(epi_comm *c);
int epi_comm_rank(const epi_comm *c);
int epi_comm_world(const epi_comm *c);
int64_t epi_comm_last_exchange_bytes(const epi_comm *c);   /* bytes this rank handed to the last report's all-reduce(s) */
/* Test hook (world size 1): treat `ntiles` consecutive tiles in the middle of the batch as shared, so that slab, collective
 * and the owners' emit run on a one-GPU box (bench.py sharded_1rank, tests). */
void epi_comm_set_test_shared(epi_comm *c, int ntiles);
int epi_batch_cytosine_report_sharded(epi_batch *b, epi_comm *c, const char *ctx_meth, const char *ctx_unmeth,
                                      const char *ooctx_meth, const char *ooctx_unmeth, uint32_t min_n_ctx,
                                      double min_ctx_meth_frac, double max_ooctx_meth_frac, const int32_t *d_pass,
                                      const char *ctx, int32_t *d_pass_out /* may be NULL */, void *stream, int64_t *nrow_out);
int epi_batch_mhl_report_sharded(epi_batch *b, epi_comm *c, const char *ctx, int hmax, int hmin, double max_ooctx_meth_frac,
                                 void *stream, int64_t *nrow_out);

/* ---- synthetic input (bench/tests; DESIGN.md "Synthetic workload") ------- */
typedef struct {
  uint64_t seed;
  int64_t n_total;        /* rows of the whole (all-ranks) stream              */
  int64_t row_first;      /* first global row generated by this call           */
  int64_t n;              /* rows generated by this call                       */
  int32_t read_len;       /* bytes per template                                */
  int32_t n_chr;
  int32_t depth;          /* genome length per chromosome = rows*read_len/depth */
  int32_t gap_from, gap_len; /* bytes [gap_from, gap_from+gap_len) are 0xFB filler (0 = none) */
} epi_synth_params;
int epi_synth_generate_dev(const epi_synth_params *p, uint8_t *d_xm, int64_t *d_off,
                           int32_t *d_rname, int32_t *d_strand, int32_t *d_start, void *stream);

/* Bytes (and strands) for rows the caller laid out itself -- off/rname/start in device memory, e.g. uniform-random
 * starts sorted on the device and ragged lengths: the same context track and methylation model, per-row
 * hashes keyed by the global row id row_first + k; every gap_every-th template (by hash, 0 = none) carries gap_len
 * filler bytes (0xFB) in its middle.  nbytes = off[n]. */
int epi_synth_fill_dev(uint64_t seed, int64_t row_first, int64_t n, const int64_t *d_off, const int32_t *d_rname,
                       const int32_t *d_start, int64_t nbytes, int32_t gap_every, int32_t gap_len,
                       uint8_t *d_xm, int32_t *d_strand, void *stream);

/* ---- profiling hooks (HIP events around the dominant kernels) ------------ */
void epi_prof_enable(int on);
/* name: "cx_tiles", "threshold", "mhl_tiles", ...; returns accumulated ms and launch count since reset */
int epi_prof_get(const char *name, double *ms_total, int64_t *launches);
void epi_prof_reset(void);
/* Test hook.  The device allocations the library owns right now, process-wide, and their bytes: every buffer of a batch,
 * a communicator or a call's scratch (not the engines' staging buffers).  A call that has returned holds none of its
 * scratch any more, and a batch or communicator that has been freed holds nothing: tests pin ownership with this. */
int epi_device_allocations(int64_t *live, int64_t *bytes);

/* Test hook.  The library's environment switches (EPIHIP_*: result-neutral hooks that steer a call onto a rarely
 * taken path) are read once per process; this re-reads them. */
void epi_options_reload(void);

#ifdef __cplusplus
}
#endif
#endif /* EPIHIP_H */
