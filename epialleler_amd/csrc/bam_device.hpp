// Everything the BAM host code (bam_pack.cpp, bam_call.cpp) asks of the device: page-locked host memory, the GPU's call of
// a window's records, the arena of mates = "anywhere" and the merge of its templates.  bam_device.cpp implements it twice:
// on the HIP runtime and the engine, and -- for the host-only build (EPI_HOST_ONLY), which has neither -- as a page-locked
// allocator that never locks and device steps that refuse with EPI_ERR_NODEVICE.  No other BAM unit calls the HIP runtime.
#pragma once
#include <memory>
#include <thread>
#include "common.hpp"

namespace epi {
namespace bam {

// The engine of a call that needs the device: the caller's, or the default one (no device: fails here, before any file
// is touched).  `why`: the entry point and what it does on the GPU, for the host-only build's refusal.
int device_engine(epi_engine **eng, const char *why);

// ---- page-locked host memory -------------------------------------------------------------------------------------------
bool pinned_alloc(size_t bytes, void **p);       // false: no usable device, or no memory to lock: the caller mallocs
void pinned_free(void *p);

// The output bytes go to page-locked memory (the upload DMAs straight from it).  Pinning ~100 MB takes tens of
// milliseconds, so it starts when the file is opened, next to the inflate / pack work, sized by an estimate; a template
// set that turns out larger is allocated at the end instead.
struct PinAhead {
  std::thread th;
  void *p = nullptr;
  size_t cap = 0;
  bool ok = false;
  ~PinAhead() { release(); }
  void wait() { if (th.joinable()) th.join(); }
  void release() {
    wait();
    if (ok && p) pinned_free(p);
    p = nullptr; ok = false;
  }
};
// pins `cap` bytes on a thread of pin's own, under the caller's current device
void pin_ahead_start(PinAhead &pin, size_t cap);

// ---- the device-side state of one call: the buffers of the windows to call, the arena of mates = "anywhere" -------------
struct DeviceState;
struct DeviceStateFree { void operator()(DeviceState *d) const; };
using DeviceStatePtr = std::unique_ptr<DeviceState, DeviceStateFree>;
DeviceStatePtr device_state_new();               // (host-only build: none)

// call_methylation.hip over one window's packed records: call_methylation_window with the state's buffers
int device_call_window(DeviceState *d, epi_engine *eng, epi_genome *g, const CallRec *recs, int64_t nrec, const uint32_t *cigar,
                       int64_t ncig, const uint8_t *seq, int64_t nseq, int64_t nxm, CallForm form, uint8_t *xm_out);

// mates = "anywhere".  The arena, on the engine's device; the engine's staging buffer k (stage_buffer) and its first
// `bytes` sent to the arena at `aoff` (stage_send); a piece larger than a staging buffer copied on its own.
int arena_reserve(DeviceState *d, epi_engine *eng, size_t bytes);
size_t arena_capacity(const DeviceState *d);
int arena_stage(epi_engine *eng, int k, uint8_t **buf, size_t *cap);
int arena_send(DeviceState *d, epi_engine *eng, int k, int64_t aoff, size_t bytes);
int arena_write(DeviceState *d, int64_t aoff, const uint8_t *src, size_t bytes);
// waits for the arena's last uploads (*t_sync: seconds), then assemble_templates.hip merges the rows into h_out
int arena_assemble(DeviceState *d, epi_engine *eng, const AsmTpl *tpl, int64_t ntpl, const AsmRec *recs, int64_t nrec, uint8_t q0,
                   int32_t trim5, int64_t nbytes, int64_t qbytes, uint8_t *h_out, double *t_sync, double *t_kernel, double *t_d2h);

}  // namespace bam
}  // namespace epi
