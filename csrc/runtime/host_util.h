// Host helpers shared by the runtime and the bindings: error checks, operand checks, roctx ranges,
// host-mapped words, the put grid, one bounded host wait and move-only owners of HIP handles.
#pragma once

#include <ATen/ATen.h>
#include <c10/hip/HIPStream.h>
#include <hip/hip_runtime.h>
#include <rocprofiler-sdk-roctx/roctx.h>

#include <algorithm>
#include <chrono>
#include <cstdlib>
#include <cstring>
#include <stdexcept>
#include <string>
#include <thread>
#include <utility>

#if defined(__x86_64__)
#include <immintrin.h>
#endif

namespace eh {

inline void hcheck(hipError_t e, const char* what) {
  if (e != hipSuccess) throw std::runtime_error(std::string(what) + ": " + hipGetErrorString(e));
}

inline void need(bool ok, const std::string& msg) {
  if (!ok) throw std::invalid_argument(msg);
}

inline void need_gpu(const at::Tensor& t, const char* name) {
  need(t.is_cuda() && t.is_contiguous(), std::string(name) + " must be a contiguous GPU tensor");
}

// the current HIP stream of a tensor's device: every entry point launches there
inline hipStream_t stream_of(const at::Tensor& t) { return c10::hip::getCurrentHIPStream(t.device().index()).stream(); }

// dtype code of an accumulator tensor: 0 fp64, 1 fp32
inline int acc_code(const at::Tensor& t) {
  if (t.scalar_type() == at::kDouble) return 0;
  if (t.scalar_type() == at::kFloat) return 1;
  throw std::invalid_argument("accumulator tensors must be float64 or float32");
}

// roctx ranges for rocprofv3 --marker-trace, enabled by ERASUREHEAD_TRACE=1.
inline bool trace_enabled() {
  static const bool on = [] {
    const char* e = std::getenv("ERASUREHEAD_TRACE");
    return e && e[0] && e[0] != '0';
  }();
  return on;
}

struct Range {
  explicit Range(const char* name) : on(trace_enabled()) {
    if (on) roctxRangePushA(name);
  }
  ~Range() {
    if (on) roctxRangePop();
  }
  bool on;
};

// Zeroed host memory the GPU can address (integrity records, abort words, probe flags).
struct HostMapped {
  void* host = nullptr;
  void* dev = nullptr;
  explicit HostMapped(size_t bytes) {
    hcheck(hipHostMalloc(&host, bytes, hipHostMallocMapped | hipHostMallocCoherent), "hipHostMalloc");
    std::memset(host, 0, bytes);
    const hipError_t e = hipHostGetDevicePointer(&dev, host, 0);
    if (e != hipSuccess) hipHostFree(host);
    hcheck(e, "hipHostGetDevicePointer");
  }
  ~HostMapped() { hipHostFree(host); }
  HostMapped(const HostMapped&) = delete;
  HostMapped& operator=(const HostMapped&) = delete;
};

// Grid of a put + signal launch (transport.hip put_signal): a block per 4096 16-byte vectors, at most 64.
inline int put_blocks(long long bytes) {
  return (int)std::max<long long>(1, std::min<long long>(64, (bytes / 16 + 4095) / 4096));
}

// The one bounded host wait: poll `done`, first with `spins` pauses, then with `sleep_us` sleeps, until
// `timeout` seconds have passed.  Returns the seconds waited, negative on timeout.
template <class Pred>
inline double wait_until(Pred&& done, double timeout, int spins = 4096, int sleep_us = 5) {
  using clk = std::chrono::steady_clock;
  const auto t0 = clk::now();
  for (int spin = 0; !done(); ++spin) {
    if (spin < spins) {
#if defined(__x86_64__)
      _mm_pause();
#endif
      continue;
    }
    if (std::chrono::duration<double>(clk::now() - t0).count() > timeout) return -1.0;
    std::this_thread::sleep_for(std::chrono::microseconds(sleep_us));
  }
  return std::chrono::duration<double>(clk::now() - t0).count();
}

// Move-only owners of a HIP event and a HIP stream.  Empty until created; destroyed WITHOUT a
// synchronise (a receive from a peer that is gone may never end), so an owner whose stream must finish
// first synchronises it in its own destructor.
template <class H, hipError_t (*Destroy)(H)>
class Handle {
 public:
  Handle() = default;
  explicit Handle(H h) : h_(h) {}
  Handle(Handle&& o) noexcept : h_(std::exchange(o.h_, nullptr)) {}
  Handle& operator=(Handle&& o) noexcept {
    std::swap(h_, o.h_);
    return *this;
  }
  ~Handle() {
    if (h_) Destroy(h_);
  }
  operator H() const { return h_; }
  H get() const { return h_; }

 private:
  H h_ = nullptr;
};
using Event = Handle<hipEvent_t, hipEventDestroy>;
using Stream = Handle<hipStream_t, hipStreamDestroy>;

// flags: hipEventDisableTiming for a pure ordering event, hipEventDefault for one that is timed
inline Event make_event(unsigned flags = hipEventDisableTiming) {
  hipEvent_t e = nullptr;
  hcheck(hipEventCreateWithFlags(&e, flags), "hipEventCreate");
  return Event(e);
}
inline Stream make_stream() {
  hipStream_t s = nullptr;
  hcheck(hipStreamCreateWithFlags(&s, hipStreamNonBlocking), "hipStreamCreate");
  return Stream(s);
}
// Record a timing event on `st`, creating it at its first use (the pumps' per-round timing).
inline void record_timed(Event& e, hipStream_t st) {
  if (!e) e = make_event(hipEventDefault);
  hcheck(hipEventRecord(e, st), "hipEventRecord");
}

}  // namespace eh
