// WorkerPump: a worker rank's per-round hot loop in C++ (GIL released), set up by engine/trainer.py.
// Reference loop (every engine, ref src/naive.py:88-150, src/approximate_coding.py:136-207):
//   worker: Wait(beta) -> gradient -> [delay] -> Isend(g)
//  WorkerPump::run(a, b)  for each round: spin on the beta round counter (or wait for its receive),
//                         launch the gradient of every local logical worker, put+signal the messages
//                         into the master's mailbox ring (or send them).
// Everything is stream-ordered on the rank's compute stream; the only host wait is the beta counter
// (IPC) or the event behind the previous beta receive (p2p).
#include <c10/hip/HIPStream.h>
#include <pybind11/stl.h>
#include <torch/extension.h>

#include <algorithm>
#include <array>
#include <cstdint>
#include <memory>
#include <string>
#include <tuple>
#include <vector>

#include "runtime/comm.h"
#include "runtime/grad_launcher.h"
#include "runtime/integrity_host.h"

namespace {
namespace py = pybind11;
using at::Tensor;
using namespace eh;

// ------------------------------------------------------------------------- WorkerPump
class WorkerPump {
 public:
  WorkerPump(std::shared_ptr<GradLauncher> g, const Tensor& inbox, const Tensor& G, int n_loc, uintptr_t mbox_base,
             int mbox_rows, int row0, uintptr_t beta_flag_host, uintptr_t msg_flag_dev, const Tensor& counters,
             int K, int device, double timeout, uintptr_t beta_flag_dev)
      : WorkerPump(std::move(g), inbox, G, n_loc, K, device, timeout) {
    need(row0 >= 0 && row0 + n_loc <= mbox_rows, "mailbox rows out of range");
    need(beta_flag_host != 0 && msg_flag_dev != 0 && mbox_base != 0, "null address");
    need(counters.is_cuda() && counters.scalar_type() == at::kInt && counters.numel() >= 1, "counters");
    mbox_ = mbox_base;
    mbox_rows_ = mbox_rows;
    row0_ = row0;
    bflag_ = reinterpret_cast<uint64_t*>(beta_flag_host);
    bflag_dev_ = reinterpret_cast<void*>(beta_flag_dev);
    mflag_ = reinterpret_cast<unsigned long long*>(msg_flag_dev);
    counters_ = counters;
    fuse_put_ = g_->can_fuse_put(n_loc);
    // Device-side beta wait: the stream itself waits for the flag (hipStreamWaitValue64 on the
    // host-registered shared flag), so round i's kernels are already queued when beta(i) lands
    // instead of after a host wake-up + launch.  The host stays one round ahead and keeps the
    // timeout.  beta_flag_dev = 0 selects the host-side wait (the caller's policy).
    int can = 0;
    if (bflag_dev_ && hipDeviceGetAttribute(&can, hipDeviceAttributeCanUseStreamWaitValue, device) == hipSuccess)
      dwait_ = can != 0;
    csum_ = at::zeros({eh::kMaxTagRows}, at::TensorOptions().dtype(at::kLong).device(at::Device(at::kCUDA, device)));
  }
  // Stream-ordered p2p worker (runtime/comm.h: RCCL, or its single-GPU loopback): every round is
  // recv(beta) -> gradient -> [late spin] -> send(messages) on this rank's stream, enqueued one round
  // ahead of the beta that has landed (the host waits on the event behind the previous receive).
  WorkerPump(std::shared_ptr<GradLauncher> g, const Tensor& inbox, const Tensor& G, int n_loc,
             std::shared_ptr<eh::P2PComm> comm, int K, int device, double timeout)
      : WorkerPump(std::move(g), inbox, G, n_loc, K, device, timeout) {
    need(comm != nullptr, "null communicator");
    comm_ = std::move(comm);
    for (auto& e : rev_) e = make_event();
  }
  bool fused_put() const { return fuse_put_; }
  bool device_wait() const { return dwait_; }
  std::string comm_kind() const { return comm_ ? comm_->kind() : "ipc"; }

  // --delay-on worker: seconds this rank is physically late in every round.  A device spin
  // (wall_clock64 + s_sleep) between the gradient and the put, so the put really leaves late
  // while the rounds stay queued; the put is then its own kernel (not fused into the reduction).
  void set_delays(const std::vector<double>& seconds) {
    need((int)seconds.size() >= R_, "delays must cover R rounds");
    int khz = 0;
    hcheck(hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, device_), "hipDeviceGetAttribute");
    late_ticks_.assign(R_, 0);
    for (int i = 0; i < R_; ++i)
      late_ticks_[i] = static_cast<long long>(std::min(seconds[i], 3600.0) * 1e3 * khz);
    if (std::any_of(late_ticks_.begin(), late_ticks_.end(), [](long long t) { return t > 0; })) fuse_put_ = false;
  }
  // --slow-ranks: the gradient runs `n` times per round.
  void set_repeat(int n) {
    need(n >= 1, "repeat must be >= 1");
    repeat_ = n;
  }

  // Drain "lazy": stale-round skipping (the replacement of the reference's send Cancel, ref
  // src/coded.py:178-180).  Every round's kernels carry a gate word (common.h gate_closed); round i's
  // put decides round i+1's: skip it iff this rank's beta counter (beta_flag_dev, its device address)
  // already says beta(i+2) is out, i.e. the master finished round i+1 before this rank could start it.
  // Decided on the device when the previous round ends, so a rank that fell behind (a late spin, a
  // slow GPU) jumps to the newest beta instead of computing stale rounds.  IPC mailbox only (RCCL has
  // no cancel: a skipped send would desynchronise the FIFO pairing).
  void set_skip_stale(uintptr_t beta_flag_dev) {
    need(!comm_, "stale-round skipping needs the IPC mailbox (p2p sends cannot be skipped)");
    need(beta_flag_dev != 0, "null beta flag");
    skip_flag_ = reinterpret_cast<const unsigned long long*>(beta_flag_dev);
    gate_ = at::zeros({R_ + 1}, at::TensorOptions().dtype(at::kInt).device(at::Device(at::kCUDA, device_)));
  }
  // The same over stream-ordered p2p (RCCL / loopback / rccl-self), where a send cannot be skipped: the
  // rank receives beta on a stream of its own, one round AHEAD of its compute (the reference pre-posts
  // every Irecv, ref src/naive.py:66-70), and bumps a device counter behind every receive (value j + 1
  // <=> beta(j) landed).  Round i's gate is snapshotted from it just before the round's gradient: closed
  // iff beta(i+1) already landed, i.e. the master decided round i before this rank could start it.  A
  // skipped round still SENDS (its stale rows keep the FIFO pairing of the master's receives) and lands
  // after its round ended, so the master drains it and never decodes it (collector.h stale arrivals).
  // The master's end-of-run beta(R) (MasterPump::finish_run) closes every round still queued.
  void set_skip_stale_comm() {
    need(comm_ != nullptr, "p2p stale-round skipping needs a communicator");
    if (skip_comm_) return;
    skip_comm_ = true;
    gate_ = at::zeros({R_ + 1}, at::TensorOptions().dtype(at::kInt).device(at::Device(at::kCUDA, device_)));
    bcount_ = at::zeros({1}, at::TensorOptions().dtype(at::kLong).device(at::Device(at::kCUDA, device_)));
    bst_ = make_stream();
    for (int j = 0; j <= R_; ++j) bev_.push_back(make_event());
  }
  bool skip_stale() const { return skip_flag_ != nullptr || skip_comm_; }

  // IPC: every message put writes {round + 1, landing ticks} into this rank's ring of shared host memory,
  // 16-byte slot i % ring (ring_dev: device address of the ring), read by the master's collector
  // (collector.h "Device times").
  void set_stamp_ring(uintptr_t ring_dev, int ring) {
    need(ring_dev == 0 || ring >= 1, "stamp ring must have >= 1 slot");
    ring_dev_ = ring_dev;
    ring_ = ring;
  }
  // Per-round device records (wall_clock64 ticks, -1 = not recorded), tests/lazy_check.py:
  //   [0] landing stamp of the round's put (IPC, written by the put kernel before its flag)
  //   [1] [2] just before / after the round's put or send      [3] [4] spin start / end (--delay-on worker)
  //   [5] [6] just before / after the stale-round gate (p2p)    [7] [8] just before / after the counter bump
  //   that announces beta(i) landed on this rank (p2p with stale-round skipping)
  //   [9] the round's start on this rank's stream: right behind its beta wait (device wait / receive), or
  //   where the host enqueued the round after its own wait -- the worker half of the master's chain
  static constexpr int kRec = 10;
  void set_records(bool on) {
    rec_ = on ? at::full({R_ + 1, kRec}, -1, at::TensorOptions().dtype(at::kLong).device(at::Device(at::kCUDA, device_)))
              : Tensor();
  }
  Tensor records() {
    hcheck(hipStreamSynchronize(stream_), "hipStreamSynchronize");
    if (bst_) hcheck(hipStreamSynchronize(bst_), "hipStreamSynchronize");
    return rec_.defined() ? rec_.cpu() : Tensor();
  }
  // Rounds this rank skipped as stale (syncs the stream).
  std::vector<int> skipped_rounds() {
    std::vector<int> out;
    if (!gate_.defined()) return out;
    hcheck(hipStreamSynchronize(stream_), "hipStreamSynchronize");
    const Tensor g = gate_.cpu();
    const int* v = g.data_ptr<int>();
    for (int i = 0; i < R_; ++i)
      if (v[i]) out.push_back(i);
    return out;
  }

  // Integrity tags (csrc/kernels/integrity.h): mbox_tags = this rank's view of the master
  // mailbox's tag slots [K][mbox_rows]; inbox_tags = its own inbox's tag slots [R + 1].  Every
  // message put carries a tag per row; every beta is checked after the round that read it.
  // Returns whether tags are on: a rank hosting more than kMaxTagRows message rows puts them untagged
  // (the caller records why) rather than failing its setup.
  bool set_integrity(uintptr_t mbox_tags, uintptr_t inbox_tags, int rank, bool on) {
    need(!on || (mbox_tags != 0 && inbox_tags != 0), "integrity tags need the tag slots");
    if (n_ > eh::kMaxTagRows) on = false;
    tags_ = on;
    mtags_ = reinterpret_cast<eh::MsgTag*>(mbox_tags);
    itags_ = reinterpret_cast<const eh::MsgTag*>(inbox_tags);
    rank_ = rank;
    return tags_;
  }
  // Raise the first failed beta check (host-mapped record), after releasing this rank's queued work.
  void check_integrity() {
    const auto* e = static_cast<const eh::IntegrityErr*>(err_.host);
    if (!__atomic_load_n(&e->flag, __ATOMIC_ACQUIRE)) return;
    stop_queued();
    throw std::runtime_error("rank " + std::to_string(rank_) + ": " + integrity_message(*e, true));
  }
  void set_timing(bool on) {
    timing_ = on;
    if (on && tev_.empty()) tev_.resize(R_);
  }
  // (beta_wait_s [R], kernel_ms [R], put_ms [R]); -1 where a round was not timed.  Syncs the stream.
  std::tuple<std::vector<double>, std::vector<double>, std::vector<double>> timing() {
    hcheck(hipStreamSynchronize(stream_), "hipStreamSynchronize");
    std::vector<double> ker(R_, -1.0), put(R_, -1.0);
    for (int i = 0; i < (int)tev_.size(); ++i) {
      const auto& t = tev_[i];
      float ms = 0.f;
      if (t[0] && t[1] && hipEventElapsedTime(&ms, t[0], t[1]) == hipSuccess) ker[i] = ms;
      if (t[1] && t[2] && hipEventElapsedTime(&ms, t[1], t[2]) == hipSuccess) put[i] = ms;
    }
    return {wait_s_, ker, put};
  }

  // Rounds [a, b).  Returns -1 when every round was issued, else the round whose beta
  // did not arrive within the timeout.
  int run(int a, int b) {
    if (comm_) return run_comm(a, b);
    py::gil_scoped_release nogil;
    for (int i = a; i < b; ++i) {
      need(i >= 0 && i < R_, "round out of range");
      Range tr("eh.worker.round");
      if (dwait_) {
        // enqueue round i once beta(i-1) is in: one round of lookahead, host timeout kept
        if (i > a && !host_wait(i, i - 1)) return release(i - 1);
        check_integrity();
        if (n_ == 0) continue;
        hcheck(hipStreamWaitValue64(stream_, bflag_dev_, static_cast<uint64_t>(i + 1), hipStreamWaitValueGte),
               "hipStreamWaitValue64(beta flag)");
      } else {
        if (!host_wait(i + 1, i)) return i;
        check_integrity();
        if (n_ == 0) continue;
      }
      stamp(i, 9, stream_);
      const int slot = i % K_;
      const char* beta = beta_row(i);
      char* g = ring_slot(i);
      const long long bytes = static_cast<long long>(n_) * ld_ * es_;
      eh::PutDesc pd{g, reinterpret_cast<char*>(mbox_) + (static_cast<int64_t>(slot) * mbox_rows_ + row0_) * ld_ * es_,
                     bytes, mflag_, static_cast<unsigned long long>(i + 1),
                     reinterpret_cast<unsigned int*>(counters_.data_ptr<int>())};
      pd.abort = static_cast<const int*>(abort_.dev);
      const int* gate = nullptr;  // stale-round gate of this round (set_skip_stale)
      if (skip_flag_) {
        int* gw = gate_.data_ptr<int>();
        gate = gw + i;
        pd.gate = gate;
        pd.next_gate = gw + i + 1;
        pd.beta_flag = skip_flag_;
        pd.stale_next = static_cast<unsigned long long>(i) + 3;  // round i+1 is stale once beta(i+2) is out
      }
      if (tags_) {
        pd.tag = mtags_ + static_cast<int64_t>(slot) * mbox_rows_ + row0_;
        pd.csum = reinterpret_cast<unsigned long long*>(csum_.data_ptr<int64_t>());
        pd.rows = n_;
        pd.es = es_;
        pd.rank = static_cast<unsigned int>(rank_);
        pd.corrupt = sabotage("msg", rank_, i) ? 1 : 0;
      }
      if (ring_dev_) pd.stamp = reinterpret_cast<long long*>(ring_dev_) + 2 * (i % ring_);
      pd.stamp_log = rec_at(i, 0);
      if (fuse_put_) {  // gradient + put + signal in one stream order, no separate put kernel
        if (timing_) record_t(i, 0);
        for (int k = 1; k < repeat_; ++k) hcheck(g_->launch(beta, g, stream_, gate), "worker gradient (slow rank)");
        hcheck(g_->launch_put(beta, g, pd, stream_), "worker gradient + put");
        if (timing_) record_t(i, 1);
        if (timing_) record_t(i, 2);
      } else {
        compute_and_send(i, beta, g, gate, skip_flag_, static_cast<unsigned long long>(R_) + 1, [&] {
          eh::PutArgs pa{};
          pa.n = 1;
          pa.d[0] = pd;
          hcheck(eh::put_signal_launch(pa, put_blocks(bytes), stream_), "put_signal(messages)");
        });
      }
      if (tags_)  // beta(i) against its tag, behind the round that read it (off the critical path)
        hcheck(eh::verify_rows_launch(beta, itags_ + i, 1, ld_, es_, static_cast<unsigned int>(i + 1), 0u,
                                      static_cast<eh::IntegrityErr*>(err_.dev), -1, stream_),
               "verify_rows(beta)");
    }
    if (dwait_ && b > a && !host_wait(b, b - 1)) return release(b - 1);
    if (skip_flag_ && b == R_ && n_ > 0)  // every round is put or skipped: the master's collector can drain
      hcheck(eh::signal_launch(mflag_, static_cast<unsigned long long>(R_), stream_), "signal(rounds done)");
    if (tags_) {  // the last rounds' checks
      hcheck(hipStreamSynchronize(stream_), "hipStreamSynchronize");
      check_integrity();
    }
    return -1;
  }

 private:
  // What both transports share.
  WorkerPump(std::shared_ptr<GradLauncher> g, const Tensor& inbox, const Tensor& G, int n_loc, int K, int device,
             double timeout)
      : g_(std::move(g)), inbox_(inbox), G_(G), n_(n_loc), K_(K), timeout_(timeout), device_(device) {
    need_gpu(inbox, "inbox");
    need_gpu(G, "G");
    need(G.dim() == 3 && G.size(0) == K && G.size(2) == inbox.size(1), "G must be [K, n, ld]");
    need(acc_code(G) == acc_code(inbox), "G/inbox dtype mismatch");
    need(n_loc >= 0 && n_loc <= G.size(1), "n_loc out of range");
    ld_ = (int)inbox.size(1);
    R_ = (int)inbox.size(0) - 1;
    es_ = acc_code(G) == 0 ? 8 : 4;
    g_rows_ = (int)G.size(1);
    stream_ = c10::hip::getCurrentHIPStream(device).stream();
    wait_s_.assign(R_, -1.0);
  }

  // Beta receives of rounds <= j on the beta stream (set_skip_stale_comm), each followed by the counter
  // bump and its event.
  void post_beta_upto(int j) {
    const int64_t bbytes = static_cast<int64_t>(ld_) * es_;
    auto* cnt = reinterpret_cast<unsigned long long*>(bcount_.data_ptr<int64_t>());
    for (; posted_ <= std::min(j, R_); ++posted_) {
      char* beta = beta_row(posted_);
      comm_->recv(0, beta, bbytes, bst_);
      stamp(posted_, 7, bst_);
      hcheck(eh::signal_launch(cnt, static_cast<unsigned long long>(posted_) + 1, bst_), "signal(beta landed)");
      stamp(posted_, 8, bst_);
      hcheck(hipEventRecord(bev_[posted_], bst_), "hipEventRecord(beta)");
    }
  }
  // run_comm with stale-round skipping (set_skip_stale_comm).
  int run_comm_skip(int a, int b) {
    py::gil_scoped_release nogil;
    if (posted_ == 0) posted_ = a;  // a resumed run: the master's first beta is beta(a)
    need(posted_ >= a, "rounds must run in order");
    auto* cnt = reinterpret_cast<const unsigned long long*>(bcount_.data_ptr<int64_t>());
    int* gw = gate_.data_ptr<int>();
    for (int i = a; i < b; ++i) {
      need(i >= 0 && i < R_, "round out of range");
      Range tr("eh.worker.round");
      if (i > a && !event_wait(bev_[i - 1], i - 1)) {  // beta(i-1) never came: the master is gone
        comm_->abort();
        return i - 1;
      }
      // beta(i+1) (or the end-of-run beta(R)) may land while round i waits.  Never past the segment: the
      // master publishes beta(b) only after the fence between segments (Trainer.run timed_start), and a
      // receive still posted would hold this rank's device synchronisation at that fence.
      post_beta_upto(b == R_ ? i + 1 : std::min(i + 1, b - 1));
      hcheck(hipStreamWaitEvent(stream_, bev_[i], 0), "hipStreamWaitEvent(beta)");
      if (n_ == 0) continue;
      stamp(i, 9, stream_);
      // closed iff beta(i+1) landed before this round starts (value i + 2)
      stamp(i, 5, stream_);
      hcheck(eh::gate_launch(cnt, static_cast<unsigned long long>(i) + 2, gw + i, stream_), "gate(stale round)");
      stamp(i, 6, stream_);
      char* g = ring_slot(i);
      // a skipped round does not spin (the end of the run stops one) but still sends: the FIFO pairing
      compute_and_send(i, beta_row(i), g, gw + i, cnt, static_cast<unsigned long long>(R_) + 1,
                       [&] { comm_->send(0, g, static_cast<int64_t>(n_) * ld_ * es_, stream_); });
    }
    if (b > a && !event_wait(bev_[b - 1], b - 1)) {
      comm_->abort();
      return b - 1;
    }
    if (b == R_) {  // the master's end-of-run beta(R): nothing may stay posted on the communicator
      post_beta_upto(R_);
      if (!event_wait(bev_[R_], R_ - 1)) {
        comm_->abort();
        return R_ - 1;
      }
    }
    return -1;
  }
  int run_comm(int a, int b) {
    if (skip_comm_) return run_comm_skip(a, b);
    py::gil_scoped_release nogil;
    const int64_t bbytes = static_cast<int64_t>(ld_) * es_;
    for (int i = a; i < b; ++i) {
      need(i >= 0 && i < R_, "round out of range");
      Range tr("eh.worker.round");
      if (i > a && !event_wait(rev_[(i - 1) % 2], i - 1)) {  // beta(i-1) never came: the master is gone
        comm_->abort();
        return i - 1;
      }
      char* beta = beta_row(i);
      comm_->recv(0, beta, bbytes, stream_);
      hcheck(hipEventRecord(rev_[i % 2], stream_), "hipEventRecord(beta)");
      if (n_ == 0) continue;
      stamp(i, 9, stream_);
      char* g = ring_slot(i);
      compute_and_send(i, beta, g, nullptr, nullptr, 0,
                       [&] { comm_->send(0, g, static_cast<int64_t>(n_) * ld_ * es_, stream_); });
    }
    if (b > a && !event_wait(rev_[(b - 1) % 2], b - 1)) {
      comm_->abort();
      return b - 1;
    }
    return -1;
  }
  // The part of a round every loop shares, behind its beta and its gate: repeat_ gradients between their
  // timing events, the late spin of --delay-on worker (after compute, before the send: ref
  // src/naive.py:141-148; it ends early once `spin_flag` reaches `spin_top`), then the round's put or
  // send between its stamps.
  template <class Send>
  void compute_and_send(int i, const char* beta, char* g, const int* gate, const unsigned long long* spin_flag,
                        unsigned long long spin_top, Send&& send) {
    if (timing_) record_t(i, 0);
    for (int k = 0; k < repeat_; ++k) hcheck(g_->launch(beta, g, stream_, gate), "worker gradient");
    if (timing_) record_t(i, 1);
    if (!late_ticks_.empty() && late_ticks_[i] > 0)
      hcheck(eh::spin_launch(late_ticks_[i], stream_, gate, spin_flag, spin_top, rec_at(i, 3)), "late worker spin");
    stamp(i, 1, stream_);
    send();
    stamp(i, 2, stream_);
    if (timing_) record_t(i, 2);
  }

  // Bounded host waits (host_util.h wait_until); the seconds waited go under round `rec`.
  bool waited(double s, int rec) {
    if (s < 0.0) return false;
    wait_s_[rec] = s;
    return true;
  }
  // until a receive event completed (comm mode)
  bool event_wait(hipEvent_t ev, int rec) {
    return waited(wait_until(
                      [ev] {
                        const hipError_t q = hipEventQuery(ev);
                        if (q != hipSuccess && q != hipErrorNotReady) hcheck(q, "hipEventQuery(beta)");
                        return q == hipSuccess;
                      },
                      timeout_),
                  rec);
  }
  // until the beta flag reaches `target`
  bool host_wait(uint64_t target, int rec) {
    return waited(wait_until([&] { return __atomic_load_n(bflag_, __ATOMIC_ACQUIRE) >= target; }, timeout_), rec);
  }
  // Timeout with device-side waits queued: the master is gone (or late beyond the timeout).  The
  // queued rounds must not announce messages computed on a beta that never arrived, so the abort
  // word goes up FIRST (every queued put / put+signal kernel checks it and skips its put and its
  // signal), then this rank's own stream waits are released (the flag value they wait for) so no
  // wait is left on the GPU.  Returns the round that timed out.
  int release(int bad) {
    stop_queued();
    return bad;
  }
  void stop_queued() {
    if (comm_) {
      comm_->abort();
      return;
    }
    __atomic_store_n(static_cast<int*>(abort_.host), 1, __ATOMIC_RELEASE);
    if (dwait_) {
      const uint64_t top = static_cast<uint64_t>(R_) + 1;
      if (__atomic_load_n(bflag_, __ATOMIC_ACQUIRE) < top) __atomic_store_n(bflag_, top, __ATOMIC_RELEASE);
    }
    hipStreamSynchronize(stream_);
  }

  void record_t(int i, int which) { record_timed(tev_[i][which], stream_); }
  // Ring slot i % K of G, and row j of the inbox.
  char* ring_slot(int i) const {
    return static_cast<char*>(G_.data_ptr()) + static_cast<int64_t>(i % K_) * g_rows_ * ld_ * es_;
  }
  char* beta_row(int j) const { return static_cast<char*>(inbox_.data_ptr()) + static_cast<int64_t>(j) * ld_ * es_; }
  // Address of record field `f` of round i (nullptr when records are off).
  long long* rec_at(int i, int f) {
    if (!rec_.defined() || i < 0 || i > R_) return nullptr;
    return reinterpret_cast<long long*>(rec_.data_ptr<int64_t>()) + static_cast<int64_t>(i) * kRec + f;
  }
  void stamp(int i, int f, hipStream_t st) {
    if (long long* p = rec_at(i, f)) hcheck(eh::stamp_launch(p, st), "stamp(record)");
  }

  std::shared_ptr<GradLauncher> g_;
  Tensor inbox_, G_;
  int n_;
  uintptr_t mbox_ = 0;
  int mbox_rows_ = 0, row0_ = 0;
  uint64_t* bflag_ = nullptr;
  void* bflag_dev_ = nullptr;
  uintptr_t ring_dev_ = 0;  // set_stamp_ring
  int ring_ = 1;
  Tensor rec_;              // set_records
  unsigned long long* mflag_ = nullptr;
  Tensor counters_;
  int K_;
  double timeout_;
  int ld_ = 0, R_ = 0, es_ = 8, g_rows_ = 1;
  hipStream_t stream_ = nullptr;
  bool timing_ = false;
  bool fuse_put_ = false;
  bool dwait_ = false;
  bool tags_ = false;
  eh::MsgTag* mtags_ = nullptr;          // master mailbox tag slots (this rank's mapping)
  const eh::MsgTag* itags_ = nullptr;    // own inbox tag slots
  int rank_ = 0;
  HostMapped err_{sizeof(eh::IntegrityErr)};      // first failed beta check (eh::IntegrityErr)
  HostMapped abort_{sizeof(int)};    // int: queued puts skip themselves once set
  Tensor csum_;                          // tagged put checksum scratch [kMaxTagRows]
  std::vector<long long> late_ticks_;    // [R] device spin before the put (--delay-on worker)
  const unsigned long long* skip_flag_ = nullptr;  // beta counter read by the stale-round gates (lazy drain)
  Tensor gate_;                          // int32 [R + 1] stale-round gates (1 = round skipped)
  bool skip_comm_ = false;               // p2p stale-round skipping (set_skip_stale_comm)
  Tensor bcount_;                        // int64 [1]: j + 1 once beta(j) landed (p2p skipping)
  Stream bst_;  // beta receive stream (p2p skipping); never synchronised at teardown: a receive from a master that is gone may never end
  std::vector<Event> bev_;               // [R + 1] beta(j) landed (p2p skipping)
  int posted_ = 0;                       // beta receives posted on bst_ so far
  int repeat_ = 1;                       // gradient launches per round (--slow-ranks)
  int device_ = 0;
  std::shared_ptr<eh::P2PComm> comm_;    // stream-ordered p2p (null: IPC mailbox)
  std::array<Event, 2> rev_;             // beta receive-done events of the last two rounds (comm mode)
  std::vector<std::array<Event, 3>> tev_;  // [round] gradient start, gradient end = put start, put end
  std::vector<double> wait_s_;                  // [round] host seconds spent waiting for beta
};

}  // namespace

namespace eh {
void bind_worker_pump(py::module& m) {
  py::class_<WorkerPump>(m, "WorkerPump")
      .def(py::init<std::shared_ptr<GradLauncher>, const Tensor&, const Tensor&, int, uintptr_t, int, int, uintptr_t,
                    uintptr_t, const Tensor&, int, int, double, uintptr_t>(),
           py::arg("g"), py::arg("inbox"), py::arg("G"), py::arg("n_loc"), py::arg("mbox_base"), py::arg("mbox_rows"),
           py::arg("row0"), py::arg("beta_flag_host"), py::arg("msg_flag_dev"), py::arg("counters"), py::arg("K"),
           py::arg("device"), py::arg("timeout"), py::arg("beta_flag_dev") = 0)
      .def(py::init<std::shared_ptr<GradLauncher>, const Tensor&, const Tensor&, int, std::shared_ptr<eh::P2PComm>, int,
                    int, double>(),
           py::arg("g"), py::arg("inbox"), py::arg("G"), py::arg("n_loc"), py::arg("comm"), py::arg("K"),
           py::arg("device"), py::arg("timeout"))
      .def_property_readonly("comm_kind", &WorkerPump::comm_kind)
      .def("run", &WorkerPump::run)
      .def_property_readonly("fused_put", &WorkerPump::fused_put)
      .def_property_readonly("device_wait", &WorkerPump::device_wait)
      .def("set_timing", &WorkerPump::set_timing)
      .def("set_delays", &WorkerPump::set_delays)
      .def("set_repeat", &WorkerPump::set_repeat)
      .def("set_skip_stale", &WorkerPump::set_skip_stale, py::arg("beta_flag_dev"))
      .def("set_skip_stale_comm", &WorkerPump::set_skip_stale_comm)
      .def_property_readonly("skip_stale", &WorkerPump::skip_stale)
      .def("skipped_rounds", &WorkerPump::skipped_rounds)
      .def("set_integrity", &WorkerPump::set_integrity, py::arg("mbox_tags"), py::arg("inbox_tags"), py::arg("rank"),
           py::arg("on"))
      .def("check_integrity", &WorkerPump::check_integrity)
      .def("timing", &WorkerPump::timing)
      .def("set_stamp_ring", &WorkerPump::set_stamp_ring, py::arg("ring_dev"), py::arg("ring"))
      .def("set_records", &WorkerPump::set_records, py::arg("on"))
      .def("records", &WorkerPump::records);
}
}  // namespace eh
