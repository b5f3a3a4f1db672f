// common.h — internal helpers shared by the dpgo and LCD halves of libkmx.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdio>
#include <string>

#include "kmx_abi.h"

namespace kmx {
void set_error(const std::string& msg);
int fail(int code, const std::string& msg);

// The detector's resident frame pool as other parts of the library read it
// (voc.hip transforms pool frames without a second upload): device pointers
// that stay valid until the pool next grows or is replaced, and the stream
// the detector's frame uploads are enqueued on. Reads the handle only.
struct LcdPoolView {
  int device = 0;
  int n_frames = 0, max_feats = 0;
  const uint32_t* desc = nullptr;  // [n_frames][max_feats][8]
  const int* n_feats = nullptr;    // [n_frames]
  hipStream_t stream = nullptr;
};
int lcd_pool_view(kmx_lcd* h, LcdPoolView* out);  // lcd.hip

// The BowVectors a vocabulary's last transform left on the device, as bow.hip
// reads them (kmx_bow_add_from_voc appends them without a host copy): frame f
// holds nnz[f] words at words / weights [f * stride ..). The pointers stay
// valid until the vocabulary's next transform; `stream` is the one the
// transform was enqueued on. n_frames == 0: no batch. Reads the handle only.
struct VocBatchView {
  int device = 0;
  int n_words = 0, n_frames = 0, stride = 0;
  const int* nnz = nullptr;         // [n_frames]
  const uint32_t* words = nullptr;  // [n_frames][stride]
  const double* weights = nullptr;  // [n_frames][stride]
  hipStream_t stream = nullptr;
};
int voc_batch_view(kmx_voc* h, VocBatchView* out);  // voc.hip
}  // namespace kmx

#define KMX_HIP(call)                                                        \
  do {                                                                       \
    hipError_t _e = (call);                                                  \
    if (_e != hipSuccess)                                                    \
      return kmx::fail(KMX_EHIP, std::string(#call) + ": " +                 \
                                     hipGetErrorString(_e));                 \
  } while (0)

#define KMX_CHECK(cond, code, msg)                  \
  do {                                              \
    if (!(cond)) return kmx::fail((code), (msg));   \
  } while (0)

// Exceptions never cross the ABI.
#define KMX_GUARD_BEGIN try {
#define KMX_GUARD_END                                                   \
  }                                                                     \
  catch (const std::bad_alloc&) {                                       \
    return kmx::fail(KMX_ENOMEM, "host allocation failed");             \
  }                                                                     \
  catch (const std::exception& ex) {                                    \
    return kmx::fail(KMX_EINVAL, ex.what());                            \
  }
