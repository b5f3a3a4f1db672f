// devbuf.h — the one owner of a device allocation: kmx::BasicDevBuf<T, Mem>,
// move-only, pointer and capacity (in elements) together. A handle's buffers
// are members of this type, so nothing lists them a second time: the handle's
// destructor frees them, a group of them resets by assigning a fresh group,
// and "build new, then commit" is a local group and a move. Mem is the
// backend, all static (common.h has the HIP one; devbuf_check.cpp runs this
// header over malloc under the host sanitizers, so it includes nothing of HIP):
//   int  alloc(void** p, size_t bytes)   0, or a kmx error code with *p null
//   void free(void* p)
//   int  copy(void* dst, const void* src, size_t bytes, const stream_t* s)
//                                        device to device; s null: synchronous
//   int  upload(void* dst, const void* src, size_t bytes, stream_t s)
//                                        host to device, asynchronous on s
// with stream_t the stream's type. A backend may leave out the functions its
// buffers never use.
#pragma once
#include <cstddef>
#include <utility>

namespace kmx {

template <class T, class Mem>
class BasicDevBuf {
 public:
  BasicDevBuf() = default;
  BasicDevBuf(const BasicDevBuf&) = delete;  // also keeps a buffer out of a kernel's argument list: pass get()
  BasicDevBuf& operator=(const BasicDevBuf&) = delete;
  BasicDevBuf(BasicDevBuf&& o) noexcept : p_(o.p_), cap_(o.cap_) {
    o.p_ = nullptr;
    o.cap_ = 0;
  }
  BasicDevBuf& operator=(BasicDevBuf&& o) noexcept {
    if (this != &o) {
      reset();
      swap(o);
    }
    return *this;
  }
  ~BasicDevBuf() { reset(); }

  T* get() const { return p_; }
  size_t cap() const { return cap_; }  // elements; 0: no buffer

  void swap(BasicDevBuf& o) noexcept {
    std::swap(p_, o.p_);
    std::swap(cap_, o.cap_);
  }

  void reset() {
    if (p_) Mem::free(p_);
    p_ = nullptr;
    cap_ = 0;
  }

  // A fresh buffer of max(count, 1) elements, contents undefined. The old
  // buffer is freed only once the new one exists: a failure changes nothing.
  int alloc(size_t count) {
    BasicDevBuf q;
    if (int rc = q.alloc_empty(count)) return rc;
    *this = std::move(q);
    return 0;
  }

  // alloc, then the upload of host[0 .. count) enqueued on s.
  int put(const T* host, size_t count, typename Mem::stream_t s) {
    BasicDevBuf q;
    if (int rc = q.alloc_empty(count)) return rc;
    if (count)
      if (int rc = Mem::upload(q.p_, host, sizeof(T) * count, s)) return rc;
    *this = std::move(q);
    return 0;
  }

  template <class Vec>  // the same from a std::vector
  int put(const Vec& host, typename Mem::stream_t s) {
    return put(host.data(), host.size(), s);
  }

  // A buffer of max(cap, 1) elements whose first `used` are the old buffer's.
  // The old one is freed after the copy; on any failure it stays, contents and all.
  int grow_keep(size_t used, size_t cap, const typename Mem::stream_t* s = nullptr) {
    BasicDevBuf q;
    if (int rc = q.alloc_empty(cap)) return rc;
    if (p_ && used)
      if (int rc = Mem::copy(q.p_, p_, sizeof(T) * used, s)) return rc;
    *this = std::move(q);
    return 0;
  }

 private:
  int alloc_empty(size_t count) {  // *this holds nothing
    const size_t c = count ? count : 1;
    void* p = nullptr;
    if (int rc = Mem::alloc(&p, sizeof(T) * c)) return rc;
    p_ = static_cast<T*>(p);
    cap_ = c;
    return 0;
  }

  T* p_ = nullptr;
  size_t cap_ = 0;
};

}  // namespace kmx
