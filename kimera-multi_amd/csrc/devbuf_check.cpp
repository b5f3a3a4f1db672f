// devbuf_check.cpp — devbuf.h (the owning device buffer every handle is made
// of) as a stand-alone program, built by `make devbuf_check` with the host
// address and undefined-behaviour sanitizers. The backend here is malloc with a
// count of live allocations and a switch that fails the k-th allocation, so
// ownership is checked by counting: who holds the one allocation after a move
// or a swap, that a failure part-way through "build aside, then commit by move"
// leaves the target as it was, and that nothing is live at exit. CPU only.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <vector>

#include "devbuf.h"

namespace {

int g_fail = 0;

#define CHECK(cond)                                                        \
  do {                                                                     \
    if (!(cond)) {                                                         \
      std::fprintf(stderr, "devbuf_check.cpp:%d: %s\n", __LINE__, #cond);  \
      ++g_fail;                                                            \
    }                                                                      \
  } while (0)

struct HostMem {
  using stream_t = int;
  // fail_at: the allocation (counted from 1 since arm) that fails; 0: none
  static int live, allocs, frees, fail_at, copies_on_stream;
  static int alloc(void** p, size_t bytes) {
    if (++allocs == fail_at) {
      *p = nullptr;
      return 7;
    }
    *p = std::malloc(bytes);  // exactly the bytes asked for: a write past them is a sanitizer report
    if (!*p) return 7;
    ++live;
    return 0;
  }
  static void free(void* p) {
    std::free(p);
    --live;
    ++frees;
  }
  static int copy(void* dst, const void* src, size_t bytes, const int* s) {
    if (s) ++copies_on_stream;
    return std::memcpy(dst, src, bytes), 0;
  }
  static int upload(void* dst, const void* src, size_t bytes, int) { return std::memcpy(dst, src, bytes), 0; }
  static void arm(int k) {  // the k-th allocation from now fails
    allocs = 0;
    fail_at = k;
  }
};
int HostMem::live = 0, HostMem::allocs = 0, HostMem::frees = 0, HostMem::fail_at = 0, HostMem::copies_on_stream = 0;

template <class T>
using Buf = kmx::BasicDevBuf<T, HostMem>;

void check_alloc_and_reset() {
  const int frees0 = HostMem::frees;
  {
    Buf<double> b;
    CHECK(b.get() == nullptr && b.cap() == 0);
    b.reset();  // nothing to free
    CHECK(HostMem::frees == frees0);
    CHECK(b.alloc(0) == 0);  // at least one element
    CHECK(b.get() != nullptr && b.cap() == 1);
    b.get()[0] = 1.5;
    CHECK(HostMem::live == 1);
    CHECK(b.alloc(5) == 0);  // the old one is freed
    CHECK(b.cap() == 5 && HostMem::live == 1 && HostMem::frees == frees0 + 1);
    for (int k = 0; k < 5; ++k) b.get()[k] = k;
    b.reset();
    CHECK(b.get() == nullptr && b.cap() == 0 && HostMem::live == 0 && HostMem::frees == frees0 + 2);
    b.reset();  // once only
    CHECK(HostMem::frees == frees0 + 2);
    CHECK(b.alloc(3) == 0);
  }  // the destructor frees it
  CHECK(HostMem::live == 0 && HostMem::frees == frees0 + 3);
}

void check_move_and_swap() {
  const int frees0 = HostMem::frees;
  Buf<int> a;
  CHECK(a.alloc(4) == 0);
  int* pa = a.get();
  Buf<int> b(std::move(a));  // move construction: one owner
  CHECK(a.get() == nullptr && a.cap() == 0 && b.get() == pa && b.cap() == 4 && HostMem::live == 1);
  Buf<int> c;
  CHECK(c.alloc(2) == 0);
  c = std::move(b);  // move assignment frees the target's own first
  CHECK(b.get() == nullptr && b.cap() == 0 && c.get() == pa && c.cap() == 4);
  CHECK(HostMem::live == 1 && HostMem::frees == frees0 + 1);
  Buf<int>& cr = c;
  c = std::move(cr);  // onto itself: nothing happens
  CHECK(c.get() == pa && c.cap() == 4 && HostMem::live == 1);
  Buf<int> d;
  CHECK(d.alloc(9) == 0);
  int* pd = d.get();
  c.swap(d);
  CHECK(c.get() == pd && c.cap() == 9 && d.get() == pa && d.cap() == 4 && HostMem::live == 2);
  Buf<int> e;
  e.swap(d);  // with an empty one
  CHECK(d.get() == nullptr && d.cap() == 0 && e.get() == pa && e.cap() == 4 && HostMem::live == 2);
  c.reset();
  e.reset();
  CHECK(HostMem::live == 0 && HostMem::frees == frees0 + 3);
}

void check_put() {
  const std::vector<int> v = {3, 1, 4, 1, 5};
  Buf<int> b;
  CHECK(b.put(v.data(), v.size(), 0) == 0);
  CHECK(b.cap() == 5 && std::memcmp(b.get(), v.data(), sizeof(int) * 5) == 0);
  const std::vector<int> w = {9, 9};
  CHECK(b.put(w, 0) == 0);  // the vector form; the old buffer is freed
  CHECK(b.cap() == 2 && b.get()[0] == 9 && b.get()[1] == 9 && HostMem::live == 1);
  const std::vector<int> none;
  CHECK(b.put(none, 0) == 0);  // nothing to upload: one element, none read
  CHECK(b.cap() == 1 && HostMem::live == 1);
  HostMem::arm(1);
  CHECK(b.put(v, 0) == 7);  // a failed put leaves the old buffer
  CHECK(b.cap() == 1 && HostMem::live == 1);
  HostMem::arm(0);
}

void check_grow_keep() {
  Buf<long long> b;
  CHECK(b.grow_keep(0, 4) == 0);  // from nothing
  CHECK(b.cap() == 4 && HostMem::live == 1);
  for (int k = 0; k < 3; ++k) b.get()[k] = 100 + k;  // three used of four
  CHECK(b.grow_keep(3, 8) == 0);
  CHECK(b.cap() == 8 && HostMem::live == 1);
  CHECK(b.get()[0] == 100 && b.get()[1] == 101 && b.get()[2] == 102);
  const int on_stream = HostMem::copies_on_stream;
  const int stream = 0;
  CHECK(b.grow_keep(3, 16, &stream) == 0);  // the copy on a stream
  CHECK(HostMem::copies_on_stream == on_stream + 1 && b.cap() == 16 && b.get()[2] == 102);
  CHECK(b.grow_keep(0, 0) == 0);  // used 0: no copy; capacity 0: one element
  CHECK(b.cap() == 1 && HostMem::live == 1);
}

void check_failures_keep_the_old() {
  Buf<int> b;
  CHECK(b.alloc(3) == 0);
  int* p = b.get();
  for (int k = 0; k < 3; ++k) p[k] = 7 * k;
  HostMem::arm(1);
  CHECK(b.alloc(100) == 7);
  CHECK(b.get() == p && b.cap() == 3 && p[0] == 0 && p[1] == 7 && p[2] == 14 && HostMem::live == 1);
  HostMem::arm(1);
  CHECK(b.grow_keep(3, 100) == 7);
  CHECK(b.get() == p && b.cap() == 3 && p[0] == 0 && p[1] == 7 && p[2] == 14 && HostMem::live == 1);
  HostMem::arm(0);
  Buf<int> e;
  HostMem::arm(1);
  CHECK(e.alloc(2) == 7);  // an empty one stays empty
  CHECK(e.get() == nullptr && e.cap() == 0);
  HostMem::arm(0);
}

// A set_graph-style call: a struct of several buffers built as a local and
// committed by move, as ChDev / CtDev / DgDev and bow.hip's sets are.
struct Group {
  Buf<int> a;
  Buf<double> b, c;
  Buf<char> d;
};

int build_group(Group* out, size_t n, int fill, bool throw_midway) {
  Group g;
  int rc;
  if ((rc = g.a.alloc(n)) || (rc = g.b.alloc(2 * n))) return rc;
  if (throw_midway) throw std::bad_alloc();  // a host vector that could not grow, on its way to KMX_GUARD_END
  if ((rc = g.c.alloc(3 * n)) || (rc = g.d.alloc(n))) return rc;
  for (size_t k = 0; k < n; ++k) g.a.get()[k] = fill;
  *out = std::move(g);
  return 0;
}

void check_group_commit() {
  const int live0 = HostMem::live;
  Group target;
  CHECK(build_group(&target, 4, 11, false) == 0);
  CHECK(HostMem::live == live0 + 4);
  int* pa = target.a.get();
  double *pb = target.b.get(), *pc = target.c.get();
  char* pd = target.d.get();
  for (int k = 1; k <= 4; ++k) {  // a failure at each allocation of the rebuild
    HostMem::arm(k);
    CHECK(build_group(&target, 64, 22, false) == 7);
    HostMem::arm(0);
    CHECK(target.a.get() == pa && target.b.get() == pb && target.c.get() == pc && target.d.get() == pd);
    CHECK(target.a.cap() == 4 && target.b.cap() == 8 && target.c.cap() == 12 && target.d.cap() == 4);
    CHECK(target.a.get()[0] == 11 && target.a.get()[3] == 11);
    CHECK(HostMem::live == live0 + 4);  // what the failed build had allocated is freed
  }
  bool caught = false;
  try {
    (void)build_group(&target, 64, 33, true);
  } catch (const std::bad_alloc&) { caught = true; }
  CHECK(caught);
  CHECK(target.a.get() == pa && target.d.get() == pd && target.a.get()[0] == 11 && HostMem::live == live0 + 4);
  CHECK(build_group(&target, 64, 44, false) == 0);  // and a build that succeeds replaces all four
  CHECK(target.a.cap() == 64 && target.a.get()[63] == 44 && HostMem::live == live0 + 4);
  target = Group();  // the whole set resets by assignment
  CHECK(target.a.get() == nullptr && target.d.cap() == 0 && HostMem::live == live0);
}

}  // namespace

int main() {
  for (void (*check)() : {check_alloc_and_reset, check_move_and_swap, check_put, check_grow_keep,
                          check_failures_keep_the_old, check_group_commit}) {
    check();
    CHECK(HostMem::live == 0);  // after each, so at exit: asserted here, whether or not a leak detector can run
  }
  if (g_fail) return std::fprintf(stderr, "devbuf_check: %d check(s) failed\n", g_fail), 1;
  std::printf("devbuf_check ok\n");
  return 0;
}
