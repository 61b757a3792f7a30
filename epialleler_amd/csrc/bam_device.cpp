// bam_device.hpp, in its two forms: the product's, on the HIP runtime and the engine, and the host-only build's
// (EPI_HOST_ONLY: the parsers and packers under the sanitizers on a CPU, no HIP runtime to link).
#include "bam_device.hpp"
#include "bam_reader.hpp"

namespace epi {
namespace bam {

#ifndef EPI_HOST_ONLY

int device_engine(epi_engine **eng, const char *) {
  if (!*eng) EPI_TRY(epi_default_engine(eng));
  return EPI_OK;
}

bool pinned_alloc(size_t bytes, void **p) {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) == hipSuccess && ndev > 0 && hipHostMalloc(p, bytes, hipHostMallocDefault) == hipSuccess) return true;
  (void)hipGetLastError();
  return false;
}
void pinned_free(void *p) { (void)hipHostFree(p); }

void pin_ahead_start(PinAhead &pin, size_t cap) {
  pin.cap = cap;
  int cur_dev = -1;                                          // the caller's device, not device 0: every rank of a multi-GPU job pins under its own GPU
  if (hipGetDevice(&cur_dev) != hipSuccess) { (void)hipGetLastError(); cur_dev = -1; }
  pin.th = std::thread([&pin, cur_dev]() {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) == hipSuccess && ndev > 0 && (cur_dev < 0 || hipSetDevice(cur_dev) == hipSuccess) &&
        hipHostMalloc(&pin.p, pin.cap, hipHostMallocDefault) == hipSuccess) pin.ok = true;
    else (void)hipGetLastError();
  });
}

struct DeviceState {
  CallWork wk;
  DevBuf arena;                                              // sized by the file's inflated bytes: a kept record's inputs are
                                                             // smaller than the record
};
void DeviceStateFree::operator()(DeviceState *d) const { delete d; }
DeviceStatePtr device_state_new() { return DeviceStatePtr(new DeviceState); }

int device_call_window(DeviceState *d, epi_engine *eng, epi_genome *g, const CallRec *recs, int64_t nrec, const uint32_t *cigar,
                       int64_t ncig, const uint8_t *seq, int64_t nseq, int64_t nxm, CallForm form, uint8_t *xm_out) {
  return call_methylation_window(eng, g, d->wk, recs, nrec, cigar, ncig, seq, nseq, nxm, form, xm_out);
}

int arena_reserve(DeviceState *d, epi_engine *eng, size_t bytes) {
  EPI_HIP(hipSetDevice(eng->device));
  return d->arena.ensure(bytes);
}
size_t arena_capacity(const DeviceState *d) { return d->arena.cap; }
int arena_stage(epi_engine *eng, int k, uint8_t **buf, size_t *cap) { return stage_buffer(eng, k, buf, cap); }
int arena_send(DeviceState *d, epi_engine *eng, int k, int64_t aoff, size_t bytes) {
  return stage_send(eng, k, d->arena.as<uint8_t>() + aoff, bytes);
}
int arena_write(DeviceState *d, int64_t aoff, const uint8_t *src, size_t bytes) {
  EPI_HIP(hipMemcpy(d->arena.as<uint8_t>() + aoff, src, bytes, hipMemcpyHostToDevice));
  return EPI_OK;
}

int arena_assemble(DeviceState *d, epi_engine *eng, const AsmTpl *tpl, int64_t ntpl, const AsmRec *recs, int64_t nrec, uint8_t q0,
                   int32_t trim5, int64_t nbytes, int64_t qbytes, uint8_t *h_out, double *t_sync, double *t_kernel, double *t_d2h) {
  const double t0 = tnow();
  EPI_HIP(hipStreamSynchronize(eng->copy_stream));           // (the arena's last uploads)
  *t_sync = tnow() - t0;
  return assemble_templates(eng, d->arena.as<uint8_t>(), tpl, ntpl, recs, nrec, q0, trim5, nbytes, qbytes, h_out, t_kernel, t_d2h);
}

#else  // EPI_HOST_ONLY: nothing is page-locked, and the entry points that need the device refuse before they read a file

int device_engine(epi_engine **, const char *why) { return fail(EPI_ERR_NODEVICE, "%s; this build has no device code", why); }

bool pinned_alloc(size_t, void **) { return false; }
void pinned_free(void *p) { free(p); }
void pin_ahead_start(PinAhead &, size_t) {}

void DeviceStateFree::operator()(DeviceState *) const {}
DeviceStatePtr device_state_new() { return DeviceStatePtr(); }

// (not reached: device_engine has refused the calls that take these steps)
static int no_device(const char *who) { return fail(EPI_ERR_NODEVICE, "%s: this build has no device code", who); }
int device_call_window(DeviceState *, epi_engine *, epi_genome *, const CallRec *, int64_t, const uint32_t *, int64_t, const uint8_t *,
                       int64_t, int64_t, CallForm form, uint8_t *) {
  return no_device(form == CALL_PACKED ? "epi_preprocess_bam_genome" : "epi_call_methylation");
}
int arena_reserve(DeviceState *, epi_engine *, size_t) { return no_device("epi_preprocess_bam_anyorder"); }
size_t arena_capacity(const DeviceState *) { return 0; }
int arena_stage(epi_engine *, int, uint8_t **, size_t *) { return no_device("epi_preprocess_bam_anyorder"); }
int arena_send(DeviceState *, epi_engine *, int, int64_t, size_t) { return no_device("epi_preprocess_bam_anyorder"); }
int arena_write(DeviceState *, int64_t, const uint8_t *, size_t) { return no_device("epi_preprocess_bam_anyorder"); }
int arena_assemble(DeviceState *, epi_engine *, const AsmTpl *, int64_t, const AsmRec *, int64_t, uint8_t, int32_t, int64_t, int64_t,
                   uint8_t *, double *, double *, double *) {
  return no_device("epi_preprocess_bam_anyorder");
}

#endif

}  // namespace bam
}  // namespace epi
