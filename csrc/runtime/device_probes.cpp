// Two probes of the device the engine and its tests read: hardware-queue independence of a set of
// streams, and this GPU's clock against the host clock.
#include <c10/hip/HIPStream.h>
#include <pybind11/stl.h>
#include <torch/extension.h>

#include <algorithm>
#include <tuple>
#include <vector>

#include "kernels/launchers.h"
#include "runtime/collector.h"
#include "runtime/host_util.h"

namespace eh {
namespace py = pybind11;

// Test probe of hardware-queue independence: a wait on its own host flag, then an event, on every given
// stream; the flags are released in REVERSE order and each stream's event must complete before the next
// release.  A stream sharing an in-order hardware queue with an earlier one stays parked behind that
// stream's unreleased wait (its event times out).  Every flag is released before returning -- also when
// a call fails half-way -- so nothing stays queued.  Returns, per stream, whether its event completed
// within `timeout` seconds of its release.
std::vector<bool> stream_wait_probe(const std::vector<uintptr_t>& streams, double timeout) {
  const size_t n = streams.size();
  HostMapped flags(sizeof(uint64_t) * std::max<size_t>(1, n));
  auto* h = static_cast<uint64_t*>(flags.host);
  auto* d = static_cast<uint64_t*>(flags.dev);
  std::vector<Event> ev(n);
  py::gil_scoped_release nogil;
  struct Release {  // before the events and the flags go: no wait may outlive its flag
    uint64_t* h;
    const std::vector<Event>& ev;
    ~Release() {
      for (size_t k = 0; k < ev.size(); ++k) __atomic_store_n(h + k, uint64_t{1}, __ATOMIC_RELEASE);
      for (const auto& e : ev)
        if (e) hipEventSynchronize(e);
    }
  } release{h, ev};
  std::vector<bool> ok(n, false);
  for (size_t k = 0; k < n; ++k) {
    hipStream_t st = reinterpret_cast<hipStream_t>(streams[k]);
    ev[k] = make_event();
    hcheck(hipStreamWaitValue64(st, d + k, 1, hipStreamWaitValueGte), "hipStreamWaitValue64(probe)");
    hcheck(hipEventRecord(ev[k], st), "hipEventRecord(probe)");
  }
  for (size_t j = 0; j < n; ++j) {
    const size_t k = n - 1 - j;
    __atomic_store_n(h + k, uint64_t{1}, __ATOMIC_RELEASE);
    ok[k] = wait_until([&] { return hipEventQuery(ev[k]) == hipSuccess; }, timeout, 0, 50) >= 0.0;
  }
  return ok;
}

// This GPU's wall_clock64 against the host clock (Collector::now): (tick0, t0, hz) such that
// t = t0 + (ticks - tick0) / hz.  A one-thread kernel stores its clock into host-mapped memory and the
// host spins until it lands; of `tries` samples the one with the shortest launch -> seen time wins (its
// t0 lags the device store by the store's visibility latency, about a microsecond).
std::tuple<double, double, double> device_clock(int device, int tries) {
  int khz = 0;
  hcheck(hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, device), "hipDeviceGetAttribute");
  need(khz > 0, "device reports no wall clock rate");
  HostMapped slot(sizeof(long long));
  auto* h = static_cast<volatile long long*>(slot.host);
  hipStream_t st = c10::hip::getCurrentHIPStream(device).stream();
  hcheck(hipStreamSynchronize(st), "hipStreamSynchronize");
  double best = 1e30, tick0 = 0.0, t0 = 0.0;
  py::gil_scoped_release nogil;
  for (int k = 0; k < std::max(1, tries); ++k) {
    *h = -1;
    const double ta = Collector::now();
    hcheck(stamp_launch(static_cast<long long*>(slot.dev), st), "stamp(clock)");
    double tb = ta;
    for (;;) {
      tb = Collector::now();
      if (*h != -1) break;
      if (tb - ta > 5.0) throw std::runtime_error("device_clock: the stamp never landed");
    }
    if (tb - ta < best) {
      best = tb - ta;
      tick0 = static_cast<double>(*h);
      t0 = tb;
    }
  }
  hcheck(hipStreamSynchronize(st), "hipStreamSynchronize");
  return {tick0, t0, 1e3 * khz};
}

void bind_device_probes(py::module& m) {
  m.def("stream_wait_probe", &stream_wait_probe, py::arg("streams"), py::arg("timeout"));
  m.def("device_clock", &device_clock, py::arg("device"), py::arg("tries") = 16,
        "(tick0, t0, hz): this GPU's wall_clock64 against the host clock, t = t0 + (ticks - tick0) / hz");
}
}  // namespace eh
