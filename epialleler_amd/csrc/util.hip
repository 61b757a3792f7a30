// Device-wide exclusive scan over u32: scan.hpp's three launches with 16 items per thread, 4096 per workgroup.  Used for
// tile offsets and output-row offsets: tiny metadata passes next to the byte-scan kernels.
#include "common.hpp"

namespace epi {

constexpr int SCAN_THREADS = 256;
constexpr int SCAN_ITEMS = 16;                       // per thread

struct U32Load {
  const uint32_t *__restrict__ in;
  __device__ uint32_t operator()(int64_t i) const { return in[i]; }
};
struct U32StoreExclusive {
  uint32_t *__restrict__ out;
  __device__ void operator()(int64_t i, uint32_t ex, uint32_t) const { out[i] = ex; }
};

// exclusive scan, in place, of nb block sums a caller produced itself (tiles.hip); total to *d_total
int scan_block_sums_inplace(uint32_t *d_bsum, int64_t nb, uint32_t *d_total, hipStream_t s) {
  return device_scan_carry<SumU32, SCAN_THREADS>(d_bsum, nb, 0u, d_total, s);
}

int scan_exclusive_u32(const uint32_t *d_in, uint32_t *d_out, int64_t n, uint32_t *d_total, DevBuf &tmp,
                       hipStream_t s) {
  if (n <= 0) {
    if (d_total) EPI_HIP(hipMemsetAsync(d_total, 0, 4, s));
    return EPI_OK;
  }
  return device_scan<SumU32, SCAN_ITEMS, SCAN_THREADS>(n, U32Load{d_in}, U32StoreExclusive{d_out}, 0u, d_total, tmp, s);
}

}  // namespace epi
