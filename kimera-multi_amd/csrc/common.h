// common.h — internal helpers shared by the dpgo and LCD halves of libkmx:
// the error channel, the views one module gives another, and what every
// handle is made of (the owning device buffer over HIP, the stream core, the
// owning event) with the one wave reduction the kernels share.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdio>
#include <string>

#include "devbuf.h"
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

namespace kmx {
// devbuf.h's backend over the HIP runtime: a failed allocation is KMX_ENOMEM, a failed copy KMX_EHIP.
struct HipMem {
  using stream_t = hipStream_t;
  static int alloc(void** p, size_t bytes) {
    const hipError_t e = hipMalloc(p, bytes);
    if (e == hipSuccess) return 0;
    *p = nullptr;
    return fail(KMX_ENOMEM, std::string("hipMalloc: ") + hipGetErrorString(e));
  }
  static void free(void* p) { (void)hipFree(p); }
  static int copy(void* dst, const void* src, size_t bytes, const hipStream_t* s) {
    if (s) KMX_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, *s));
    else KMX_HIP(hipMemcpy(dst, src, bytes, hipMemcpyDeviceToDevice));
    return 0;
  }
  static int upload(void* dst, const void* src, size_t bytes, hipStream_t s) {
    KMX_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, s));
    return 0;
  }
};
template <class T>
using DevBuf = BasicDevBuf<T, HipMem>;

// Pinned host memory under the same owner (it is only allocated and freed).
struct HipPinned {
  using stream_t = hipStream_t;
  static int alloc(void** p, size_t bytes) {
    if (hipHostMalloc(p, bytes, hipHostMallocDefault) == hipSuccess) return 0;
    *p = nullptr;
    return fail(KMX_ENOMEM, "hipHostMalloc failed");
  }
  static void free(void* p) { (void)hipHostFree(p); }
};
template <class T>
using PinnedBuf = BasicDevBuf<T, HipPinned>;

// Pinned host memory the device reads and writes in place (mapped, coherent).
// A failed allocation is KMX_EHIP, as where the handles made these by hand.
struct HipMapped {
  using stream_t = hipStream_t;
  static int alloc(void** p, size_t bytes) {
    const hipError_t e = hipHostMalloc(p, bytes, hipHostMallocMapped | hipHostMallocCoherent);
    if (e == hipSuccess) return 0;
    *p = nullptr;
    return fail(KMX_EHIP, std::string("hipHostMalloc: ") + hipGetErrorString(e));
  }
  static void free(void* p) { (void)hipHostFree(p); }
};
template <class T>
using MappedBuf = BasicDevBuf<T, HipMapped>;  // kernels that take the host pointer itself use this alone

// A mapped buffer with its device pointer, looked up once per allocation:
// host() for the CPU, dev() for kernel arguments, cap() in elements.
template <class T>
class Mapped {
 public:
  int alloc(size_t count) {
    MappedBuf<T> q;
    void* d = nullptr;
    if (int rc = q.alloc(count)) return rc;
    KMX_HIP(hipHostGetDevicePointer(&d, q.get(), 0));
    buf_ = std::move(q);
    dev_ = static_cast<T*>(d);
    return 0;
  }
  T* host() const { return buf_.get(); }
  T* dev() const { return buf_.get() ? dev_ : nullptr; }
  size_t cap() const { return buf_.cap(); }

 private:
  MappedBuf<T> buf_;
  T* dev_ = nullptr;
};

// What every handle begins with. A handle derives from it, so the stream is
// made before the handle's buffers and events and destroyed after them.
struct StreamCore {
  int device = 0;
  hipStream_t stream = nullptr;
  bool own_stream = false;
  StreamCore() = default;
  StreamCore(const StreamCore&) = delete;
  StreamCore& operator=(const StreamCore&) = delete;
  ~StreamCore() { close(); }

  // kmx_*_create: checks the ordinal, makes the device current, creates the handle's own non-blocking stream.
  int open(int dev) {
    int ndev = 0;
    KMX_HIP(hipGetDeviceCount(&ndev));
    KMX_CHECK(dev >= 0 && dev < ndev, KMX_EINVAL, "bad HIP device ordinal");
    KMX_HIP(hipSetDevice(dev));
    device = dev;
    KMX_CHECK(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking) == hipSuccess, KMX_EHIP,
              "hipStreamCreate failed");
    own_stream = true;
    return 0;
  }
  // kmx_*_set_stream: a stream of the handle's own is synchronised and
  // destroyed, a borrowed one synchronised only if sync_borrowed; then s is held.
  int adopt(void* s, bool sync_borrowed) {
    KMX_HIP(hipSetDevice(device));
    if (stream && (own_stream || sync_borrowed)) KMX_HIP(hipStreamSynchronize(stream));
    if (stream && own_stream) KMX_HIP(hipStreamDestroy(stream));
    own_stream = false;
    stream = reinterpret_cast<hipStream_t>(s);
    return 0;
  }
  // Destroys a stream of the handle's own. Whoever deletes the handle has
  // synchronised first (destroy, below); a create that fails has enqueued nothing.
  void close() {
    if (stream && own_stream) (void)hipStreamDestroy(stream);
    stream = nullptr;
    own_stream = false;
  }
};

// kmx_*_destroy: the device current, the stream's work done, then the members free what they hold.
template <class H>
int destroy(H* h) {
  if (!h) return KMX_OK;
  (void)hipSetDevice(h->device);
  if (h->stream) (void)hipStreamSynchronize(h->stream);
  delete h;
  return KMX_OK;
}

// One owned non-blocking side stream (null until create), beside the handle's own in StreamCore.
class Stream {
 public:
  Stream() = default;
  Stream(Stream&& o) noexcept : s_(o.s_) { o.s_ = nullptr; }
  Stream& operator=(Stream&&) = delete;
  ~Stream() {
    if (s_) (void)hipStreamDestroy(s_);
  }
  int create() {
    const hipError_t e = hipStreamCreateWithFlags(&s_, hipStreamNonBlocking);
    if (e == hipSuccess) return 0;
    s_ = nullptr;
    return fail(KMX_EHIP, std::string("hipStreamCreate: ") + hipGetErrorString(e));
  }
  operator hipStream_t() const { return s_; }

 private:
  hipStream_t s_ = nullptr;
};

// One owned event (null until create); arrays and vectors of it replace the create / destroy loops.
class Event {
 public:
  Event() = default;
  Event(Event&& o) noexcept : e_(o.e_) { o.e_ = nullptr; }
  Event& operator=(Event&&) = delete;
  ~Event() {
    if (e_) (void)hipEventDestroy(e_);
  }
  int create(unsigned flags = hipEventDefault) {
    if (e_) return 0;  // (a retry after a create_events that failed part-way)
    if (hipEventCreateWithFlags(&e_, flags) == hipSuccess) return 0;
    e_ = nullptr;
    return fail(KMX_EHIP, "hipEventCreate failed");
  }
  operator hipEvent_t() const { return e_; }

 private:
  hipEvent_t e_ = nullptr;
};
template <size_t N>
int create_events(Event (&ev)[N]) {
  for (Event& e : ev)
    if (int rc = e.create()) return rc;
  return 0;
}

#ifdef __HIPCC__
// The 64-lane sum in a fixed tree; lane 0 holds it.
template <class T>
__device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  return v;
}
#endif
}  // namespace kmx
