// MasterPump: the master's per-round hot loop in C++ (GIL released), set up by engine/trainer.py.
// Reference loop (every engine, ref src/naive.py:88-150, src/approximate_coding.py:136-207):
//   master: Isend beta to all -> Waitany until the stop rule -> decode -> GD/AGD update
//  MasterPump::finish(i)  wait for the stop rule (Collector) -> decode on the host (decode.h)
//                         -> combine+update launch -> [drain] -> begin(i+1): push beta(i+1) to every
//                         worker inbox (put+signal), launch the master's own workers' gradient,
//                         register the round's arrival probes.
// Everything is stream-ordered on the rank's compute stream; the only host wait is the collector's poll.
#include <c10/hip/HIPStream.h>
#include <pybind11/stl.h>
#include <torch/extension.h>

#include <algorithm>
#include <array>
#include <cstdint>
#include <map>
#include <memory>
#include <set>
#include <stdexcept>
#include <string>
#include <tuple>
#include <vector>

#include "kernels/arbiter.h"
#include "runtime/collector.h"
#include "runtime/comm.h"
#include "runtime/decode.h"
#include "runtime/grad_launcher.h"
#include "runtime/integrity_host.h"

namespace {
namespace py = pybind11;
using at::Tensor;
using namespace eh;

// One buffer row a decode uses: its address, coefficient and, for a mailbox row, its row index
// (its integrity tag; -1 for a local row).
struct Used {
  const void* p;
  double c;
  int row;
};
using UsedRows = std::vector<Used>;

// ------------------------------------------------------------------------- MasterPump
class MasterPump {
 public:
  MasterPump(eh::Collector* col, int W, int R, int K, int d, int ld, int device, double timeout)
      : col_(col), W_(W), R_(R), K_(K), d_(d), ld_(ld), device_(device), timeout_(timeout) {
    need(col != nullptr, "collector required");
    need(W > 0 && R > 0 && K > 0 && ld >= d && d > 0, "bad pump dimensions");
    stream_ = c10::hip::getCurrentHIPStream(device).stream();
    t_start_.assign(R, 0.0);
    upd_ev_.resize(R);
    for (int k = 0; k < K; ++k) loc_ev_.push_back(make_event());
    index_.assign(2 * W, {});
    const auto i64 = at::TensorOptions().dtype(at::kLong).device(at::Device(at::kCUDA, device));
    csum_ = at::zeros({eh::kMaxPuts * eh::kMaxTagRows}, i64);  // beta put checksums
  }
  // Everything else is plain ownership (host_util.h Event / Stream, destroyed without a synchronise: a
  // receive from a dead peer may never end, the transport aborts its communicator at close).
  ~MasterPump() {
    if (chk_stream_) hipStreamSynchronize(chk_stream_);  // before its events go
    if (dev_stream_) hipStreamSynchronize(dev_stream_);  // before its graphs go
    for (auto g : graphs_) hipGraphExecDestroy(g);
  }

  // Per-round HIP-event timing of the beta puts and the local gradient launch (bench.py's
  // per-rank breakdown); off by default: each record costs the host about a microsecond.
  void set_timing(bool on) {
    timing_ = on;
    if (on && tev_.empty()) tev_.resize(R_);
  }
  // (put_ms [R], kernel_ms [R]); -1 where a round was not timed.  Syncs the stream.
  std::pair<std::vector<double>, std::vector<double>> timing_ms() {
    hcheck(hipStreamSynchronize(stream_), "hipStreamSynchronize");
    std::vector<double> put(R_, -1.0), ker(R_, -1.0);
    for (int i = 0; i < (int)tev_.size(); ++i) {
      const auto& t = tev_[i];
      float ms = 0.f;
      if (t[0] && t[1] && hipEventElapsedTime(&ms, t[0], t[1]) == hipSuccess) put[i] = ms;
      if (t[2] && t[3] && hipEventElapsedTime(&ms, t[2], t[3]) == hipSuccess) ker[i] = ms;
    }
    return {put, ker};
  }

  void set_state(const Tensor& beta, const Tensor& u, const Tensor& hist, const Tensor& beta_in) {
    arb_ready_ = false;  // the device arbiter copies this state
    for (auto* t : {&beta, &u, &hist, &beta_in}) need_gpu(*t, "beta / u / hist / beta_in");
    need(beta.scalar_type() == at::kDouble && u.scalar_type() == at::kDouble && hist.scalar_type() == at::kDouble,
         "beta/u/hist must be float64");
    need(beta.numel() == ld_ && u.numel() == ld_, "beta/u must have ld elements");
    need(hist.dim() == 2 && hist.size(0) >= R_ && hist.size(1) == ld_, "hist must be [R, ld]");
    need(beta_in.dim() == 2 && beta_in.size(0) >= R_ + 1 && beta_in.size(1) == ld_, "beta_in must be [R+1, ld]");
    beta_ = beta;
    u_ = u;
    hist_ = hist;
    beta_in_ = beta_in;
    acc_ = acc_code(beta_in);
    es_ = acc_ == 0 ? 8 : 4;
  }

  // local messages: row order of G ([K, n_loc, ld]); each (worker, part).  A (worker, part) may
  // appear several times (partition shards of one message): decode sums all its rows.
  void set_local(std::shared_ptr<GradLauncher> g, const Tensor& G, const std::vector<std::pair<int, int>>& msgs) {
    arb_ready_ = false;  // the device arbiter copies this state
    need_gpu(G, "G");
    need(G.dim() == 3 && G.size(0) == K_ && G.size(2) == ld_, "G must be [K, n_loc, ld]");
    need(acc_code(G) == acc_, "G dtype must match beta_in");
    need((int64_t)msgs.size() <= G.size(1), "more local messages than G rows");
    launcher_ = std::move(g);
    G_ = G;
    n_loc_ = (int)msgs.size();
    g_rows_ = (int)G.size(1);
    local_.clear();
    for (auto& ix : index_)
      ix.erase(std::remove_if(ix.begin(), ix.end(), [](const std::pair<int, int>& e) { return e.first == 0; }),
               ix.end());
    for (int j = 0; j < n_loc_; ++j) {
      check_wp(msgs[j].first, msgs[j].second);
      local_.push_back({msgs[j].first, msgs[j].second, j, 0});
      index_[2 * msgs[j].first + msgs[j].second].push_back({0, j});
    }
  }

  // remote messages: (worker, part, mailbox row, host address of the sender's round counter, sender rank)
  void set_remote(const Tensor& rbuf, const std::vector<std::tuple<int, int, int, uintptr_t, int>>& msgs) {
    arb_ready_ = false;  // the device arbiter copies this state
    need_gpu(rbuf, "rbuf");
    need(rbuf.dim() == 3 && rbuf.size(0) == K_ && rbuf.size(2) == ld_, "rbuf must be [K, rows, ld]");
    need(acc_code(rbuf) == acc_, "rbuf dtype must match beta_in");
    rbuf_ = rbuf;
    r_rows_ = (int)rbuf.size(1);
    remote_.clear();
    row_rank_.assign(r_rows_, 0);
    for (auto& ix : index_)
      ix.erase(std::remove_if(ix.begin(), ix.end(), [](const std::pair<int, int>& e) { return e.first == 1; }),
               ix.end());
    for (const auto& [w, p, row, addr, rank] : msgs) {
      check_wp(w, p);
      need(row >= 0 && row < r_rows_, "mailbox row out of range");
      need(addr != 0 || comm_, "null flag address");
      need(rank > 0 && rank < 256, "sender rank out of range");
      remote_.push_back({w, p, row, addr});
      row_rank_[row] = rank;
      index_[2 * w + p].push_back({1, row});
    }
  }

  // Stream-ordered p2p instead of the IPC mailbox (runtime/comm.h: RCCL, or its single-GPU loopback):
  // ranks = (worker rank, first mailbox row, rows) of every rank that sends messages; `peers` = every
  // worker rank (each receives beta).  Call after set_skip_stale, before set_remote.  beta(i) goes out
  // with one send per peer on that peer's own stream; round i's messages of rank r arrive with one
  // receive into its mailbox rows, and the HIP event behind it is the collector's probe.
  //
  // Streams (each parks its own waits: a stream that shares a hardware queue would hold back the
  // other streams of that queue, so the count must stay within GPU_MAX_HW_QUEUES):
  //   drain all / carry  ONE link stream per peer, beta(i) send then round i's receive.  Per pair this
  //                      is the order both sides need anyway (a worker cannot use beta(i+1) before it
  //                      has sent round i), and a late peer still blocks only its own link: W - 1 + the
  //                      compute stream, 8 at 8 ranks.
  //   lazy               a send and a receive stream per peer: beta(i+1) must reach a late rank while its
  //                      round-i receive is still pending, so it can find round i stale (WorkerPump::
  //                      set_skip_stale_comm): 2 (W - 1) + 1, 15 at 8 ranks.
  void set_comm(std::shared_ptr<eh::P2PComm> comm, const std::vector<std::tuple<int, int, int>>& ranks,
                const std::vector<int>& peers) {
    need(comm != nullptr, "null communicator");
    arb_ready_ = false;
    comm_ = std::move(comm);
    comm_ranks_ = ranks;
    comm_peers_ = peers;
    auto mk = [this] {
      comm_own_.push_back(make_stream());
      return static_cast<hipStream_t>(comm_own_.back());
    };
    for (int r : peers) send_st_[r] = mk();
    for (const auto& [r, row0, n] : ranks) {
      need(n > 0 && row0 >= 0, "bad mailbox rows of a rank");
      if (!skip_ && send_st_.count(r))
        recv_st_[r] = send_st_.at(r);  // the pair's link stream
      else
        recv_st_[r] = mk();
    }
    rev_.clear();
    for (size_t k = 0; k < static_cast<size_t>(K_) * ranks.size(); ++k) rev_.push_back(make_event());
    if (!bev_) bev_ = make_event();
  }
  std::string comm_kind() const { return comm_ ? comm_->kind() : "ipc"; }

  // Integrity tags (csrc/kernels/integrity.h): mbox_tags = device address of the mailbox's tag
  // slots [K][rows]; inbox_tag_off = bytes from a worker inbox base to its tag slots [R + 1].
  // on = false keeps the transport untagged (A/B runs).
  void set_integrity(uintptr_t mbox_tags, int64_t inbox_tag_off, bool on) {
    arb_ready_ = false;
    need(!on || (mbox_tags != 0 && inbox_tag_off > 0), "integrity tags need the tag slots");
    tags_ = on;
    mbox_tags_ = mbox_tags;
    inbox_tag_off_ = inbox_tag_off;
  }
  bool integrity() const { return tags_; }

  // Raise the first integrity failure any deferred check of this pump reported (host-mapped record).
  int64_t check_rows_cut() const { return check_rows_cut_; }
  void check_integrity() const {
    const auto* e = static_cast<const eh::IntegrityErr*>(err_.host);
    if (__atomic_load_n(&e->flag, __ATOMIC_ACQUIRE)) throw std::runtime_error(integrity_message(*e, false));
  }
  // End of a run: check the last round's rows too, then raise any failure.  Syncs the stream.
  void final_check() {
    flush_check();
    hcheck(hipStreamSynchronize(stream_), "hipStreamSynchronize");
    check_integrity();
  }

  // Device-side drain (after_combine): (host address, device address) of every worker rank's
  // message flag.  Empty = the host drains before pushing the next beta.
  // Returns whether the device-side drain is on (off when the device cannot wait on a value).
  bool set_drain_flags(const std::vector<std::pair<uintptr_t, uintptr_t>>& flags) {
    for (const auto& f : flags) need(f.first != 0 && f.second != 0, "null drain flag");
    int can = 0;
    const bool ok = hipDeviceGetAttribute(&can, hipDeviceAttributeCanUseStreamWaitValue, device_) == hipSuccess && can;
    drain_flags_ = ok ? flags : std::vector<std::pair<uintptr_t, uintptr_t>>{};
    return ok && !flags.empty();
  }

  // beta pushes: (inbox base device pointer [R+1, ld], flag device address) per worker rank
  void set_puts(const std::vector<std::pair<uintptr_t, uintptr_t>>& targets, const Tensor& counters) {
    arb_ready_ = false;  // the device arbiter copies this state
    need(counters.is_cuda() && counters.scalar_type() == at::kInt && counters.numel() >= (int64_t)targets.size(),
         "counters must be int32 GPU [>= n targets]");
    for (const auto& t : targets) need(t.first != 0 && t.second != 0, "null put target");
    targets_ = targets;
    counters_ = counters;
  }

  void set_schedule(const std::vector<double>& decay, const std::vector<double>& gm, const std::vector<double>& l2,
                    const std::vector<double>& theta, int update_rule, const std::vector<double>& delays, int stop_rule,
                    int k, bool drain) {
    arb_ready_ = false;  // the device arbiter copies this state
    need((int)decay.size() >= R_ && (int)gm.size() >= R_ && (int)l2.size() >= R_ && (int)theta.size() >= R_,
         "schedule arrays must cover R rounds");
    need((int64_t)delays.size() >= (int64_t)R_ * W_, "delays must be [R*W]");
    decay_ = decay;
    gm_ = gm;
    l2_ = l2;
    theta_ = theta;
    update_rule_ = update_rule;
    delays_ = delays;
    stop_rule_ = stop_rule;
    k_ = k;
    drain_ = drain;
  }

  // Multi-model run (kernels/grad_multimodel.hip): the model is M blocks of block_ld columns (d_x of them data)
  // and block k of round i takes decay / gm / l2 [i * M + k]; theta and the rule stay set_schedule's.  From
  // then on combine() launches combine_update_blocks, and the rounds cannot run on the device arbiter.
  void set_block_schedule(int M, int block_ld, int d_x, const std::vector<double>& decay, const std::vector<double>& gm,
                          const std::vector<double>& l2) {
    arb_ready_ = false;
    need(M >= 2 && M <= eh::kMaxBlocks, "block schedule: 2..8 models");
    need(block_ld >= 1 && d_x >= 1 && d_x <= block_ld && static_cast<int64_t>(M) * block_ld == ld_ && d_ == ld_,
         "block schedule: models * block_ld must be the model length");
    const size_t n = static_cast<size_t>(R_) * M;
    need(decay.size() >= n && gm.size() >= n && l2.size() >= n, "block schedule arrays must be [R * models]");
    blocks_ = M;
    block_ld_ = block_ld;
    block_dx_ = d_x;
    bdecay_ = decay;
    bgm_ = gm;
    bl2_ = l2;
  }

  // L1 / elastic net: round i ends with the soft threshold thr[i] (one model) or thr[i * M + k] (block k of a
  // multi-model run; call after set_block_schedule).  From then on combine() launches combine_update_prox with the
  // coefficients of set_schedule / set_block_schedule, and the rounds take neither fused update path (the device
  // arbiter, the slab reduction's update), as a multi-model run takes neither.
  void set_prox_schedule(const std::vector<double>& thr) {
    arb_ready_ = false;
    const size_t n = static_cast<size_t>(R_) * (blocks_ ? blocks_ : 1);
    need(thr.size() == n, "prox schedule must be [R] or [R * models]");
    for (double t : thr) need(t >= 0.0, "prox schedule: thresholds must be >= 0 (and not NaN)");
    need(n > 0, "prox schedule: no rounds");
    prox_ = thr;
  }

  // --delay-on worker: virtual delays the collector applies to REMOTE messages (the worker ranks
  // are physically late themselves); default: the same table as the local messages.
  void set_remote_delays(const std::vector<double>& delays) {
    arb_ready_ = false;
    need((int64_t)delays.size() >= (int64_t)R_ * W_, "remote delays must be [R*W]");
    remote_delays_ = delays;
  }
  // Device times of physically late ranks' messages (collector.h "Device times").  IPC: worker rank r's
  // puts write {round + 1, landing ticks} into 16-byte ring slots [r][i % ring] of shared host memory (ring_host) on
  // that rank's GPU clock clocks[r] = (tick0, t0, hz).  p2p: the receive events become timing events,
  // read against a reference event of this GPU calibrated against the host clock here.
  void set_device_times(const std::vector<std::tuple<int, double, double, double>>& clocks, uintptr_t ring_host,
                        int ring) {
    need(ring >= 1 || comm_, "stamp ring must have >= 1 slot");
    dev_times_ = true;
    for (const auto& [r, tick0, t0, hz] : clocks) {
      need(hz > 0.0, "device clock rate must be > 0");
      clocks_[r] = eh::DeviceClock{tick0, t0, hz};
    }
    ring_host_ = ring_host;
    ring_ = ring;
    if (comm_) {
      for (auto& e : rev_) e = make_event(hipEventDefault);  // timing events: the collector reads their device times
      calibrate_ref_event();
    }
  }
  // Per-round device records (tests/lazy_check.py): [R + 1][2] wall_clock64 stamps just before and just
  // after round j's beta put kernels (-1: not put by put_beta, e.g. released by the arbiter).
  void set_records(bool on) {
    rec_ = on ? at::full({R_ + 1, 2}, -1, at::TensorOptions().dtype(at::kLong).device(at::Device(at::kCUDA, device_)))
              : Tensor();
  }
  Tensor records() {
    hcheck(hipStreamSynchronize(stream_), "hipStreamSynchronize");
    return rec_.defined() ? rec_.cpu() : Tensor();
  }
  py::list probe_log() const {
    py::list out;
    for (const auto& r : col_->probe_log()) out.append(py::make_tuple(r.worker, r.part, r.round, r.t_seen, r.outcome));
    return out;
  }
  // Drain "lazy" (engine/trainer.py): the collector skips stale virtual rounds (collector.h) and, with
  // IPC targets, finish_run() tells every worker rank the run is over so its queued rounds are stale.
  void set_skip_stale(bool on) {
    need(!(on && comm_ && !comm_streams_split()), "set_skip_stale(true) after set_comm: the link streams are shared");
    skip_ = on;
    col_->set_skip_stale(on);
  }
  // Whether every peer's receive has a stream of its own (lazy drain) rather than the pair's link stream.
  bool comm_streams_split() const {
    for (const auto& [r, st] : recv_st_)
      if (send_st_.count(r) && send_st_.at(r) == st) return false;
    return true;
  }
  // The compute stream and every distinct comm stream, in creation order (tests: stream_wait_probe).
  std::vector<uintptr_t> stream_handles() const {
    std::vector<uintptr_t> out{reinterpret_cast<uintptr_t>(stream_)};
    std::set<hipStream_t> seen;
    for (const auto* m : {&send_st_, &recv_st_})
      for (const auto& [r, st] : *m)
        if (seen.insert(st).second) out.push_back(reinterpret_cast<uintptr_t>(st));
    return out;
  }
  // Distinct comm streams this pump created (rank_report: hardware-queue budget).
  int comm_streams() const {
    std::set<hipStream_t> all;
    for (const auto& [r, st] : send_st_) all.insert(st);
    for (const auto& [r, st] : recv_st_) all.insert(st);
    return static_cast<int>(all.size());
  }
  // End of the master's rounds (stream-ordered after its last beta put): with skip_stale on, every
  // worker's beta counter goes to R + 1 (as if beta(R) were out), so whatever a late worker rank still
  // has queued is stale and skipped (its gate), and its final signal lets the collector drain.
  void finish_run() {
    if (!skip_) return;
    col_->end_run(eh::Collector::now());
    if (comm_) {  // p2p: the end-of-run beta(R) to every message-sending rank (WorkerPump::run_comm_skip's last wait)
      put_beta_comm(R_, true);
      return;
    }
    for (const auto& t : targets_)
      hcheck(eh::signal_launch(reinterpret_cast<unsigned long long*>(t.second), static_cast<unsigned long long>(R_) + 1,
                               stream_),
             "signal(end of run)");
  }
  int skipped() const { return col_->skipped(); }
  int stale_arrivals() const { return col_->stale_arrivals(); }
  // --slow-ranks: this rank launches its local gradient `n` times per round (a slower GPU).
  void set_repeat(int n) {
    need(n >= 1, "repeat must be >= 1");
    repeat_ = n;
  }

  void set_decode(int kind, const std::vector<int>& group_of, int n_groups) {
    arb_ready_ = false;  // the device arbiter copies this state
    need((int)group_of.size() == W_, "group_of must have W entries");
    need(!(table_decode(kind) && W_ > 64), "table decode supports at most 64 workers");
    decode_kind_ = kind;
    group_of_ = group_of;
    n_groups_ = n_groups;
  }
  void add_table(uint64_t mask, const std::vector<double>& coefs) {
    arb_ready_ = false;  // the device arbiter copies this state
    need((int)coefs.size() == W_, "table row must have W coefficients");
    table_[mask] = coefs;
  }

  // ---- round execution ---------------------------------------------------------------
  void begin(int i) {
    Range tr("eh.master.begin");
    need(i >= 0 && i < R_, "round out of range");
    need(beta_in_.defined(), "set_state first");
    const int slot = i % K_;
    if (i >= K_ && !col_->wait_seen(i - K_, timeout_))  // the ring slot's previous round must have landed
      throw std::runtime_error("MasterPump round " + std::to_string(i) + ": messages of round " +
                               std::to_string(i - K_) + " still in flight after the round timeout; mailbox slot " +
                               std::to_string(slot) + " cannot be reused");
    const double t = eh::Collector::now();
    col_->begin_round(i, t, stop_rule_, k_);
    t_start_[i] = t;
    const void* src = beta_row(i);
    if (i != prepub_) put_beta(i);  // else already queued behind the device-side drain of round i-1
    const double* dl = delays_.data() + static_cast<int64_t>(i) * W_;
    const double* dr = remote_delays_.empty() ? dl : remote_delays_.data() + static_cast<int64_t>(i) * W_;
    if (n_loc_ > 0 && launcher_) {
      char* g = ring_slot(G_, g_rows_, i);
      if (timing_) record_t(i, 2);
      for (int k = 0; k < repeat_; ++k) hcheck(launcher_->launch(src, g, stream_), "local gradient");
      if (timing_) record_t(i, 3);
      hcheck(hipEventRecord(loc_ev_[slot], stream_), "hipEventRecord");
      for (const auto& m : local_)
        col_->add_event_probe(m.w, m.p, i, reinterpret_cast<uintptr_t>(loc_ev_[slot].get()), dl[m.w]);
    }
    flush_check();  // round i-1's mailbox rows, behind this round's beta and local gradient
    if (comm_) {  // one receive per sending rank into its mailbox rows; the event behind it is the probe
      char* rb = ring_slot(rbuf_, r_rows_, i);
      for (size_t k = 0; k < comm_ranks_.size(); ++k) {
        const auto& [r, row0, n] = comm_ranks_[k];
        hipStream_t rs = recv_st_.at(r);
        comm_->recv(r, rb + static_cast<int64_t>(row0) * ld_ * es_, static_cast<int64_t>(n) * ld_ * es_, rs);
        hipEvent_t ev = rev_[static_cast<size_t>(slot) * comm_ranks_.size() + k];
        hcheck(hipEventRecord(ev, rs), "hipEventRecord(recv)");
        for (const auto& m : remote_)
          if (m.row >= row0 && m.row < row0 + n)
            col_->add_event_probe(m.w, m.p, i, reinterpret_cast<uintptr_t>(ev), dr[m.w], !remote_delays_.empty(),
                                  dev_times_ && !remote_delays_.empty() ? reinterpret_cast<uintptr_t>(ref_ev_.get()) : 0,
                                  ref_t_);
      }
      return;
    }
    for (const auto& m : remote_) {  // physically late ranks (remote delays set): seen = arrived
      const bool physical = !remote_delays_.empty();
      uintptr_t stamp = 0;
      eh::DeviceClock clk{};
      const int r = row_rank_[m.row];
      if (physical && dev_times_ && ring_host_ && clocks_.count(r)) {  // its landing time on its own GPU clock
        stamp = ring_host_ + 2 * sizeof(int64_t) * (static_cast<uintptr_t>(r) * ring_ + i % ring_);
        clk = clocks_.at(r);
      }
      col_->add_flag_probe(m.w, m.p, i, m.flag, static_cast<uint64_t>(i + 1), dr[m.w], physical, stamp, clk);
    }
  }

  // Returns (status, arrivals [(worker, part, t_rel)], t_start, t_decoded, t_end, t_waited):
  // status 0 ok, 1 timeout (decoded with what arrived), 2 host decode needed (no table
  // row: call resolve()).
  py::tuple finish(int i, bool publish_next) {
    int status;
    std::vector<eh::Arrival> arr;
    double t_dec = 0, t_end = 0;
    {
      py::gil_scoped_release nogil;
      bool ok;
      {
        Range tr("eh.master.wait");
        ok = col_->wait(timeout_);
      }
      t_waited_ = eh::Collector::now();
      check_integrity();  // an earlier round's combine found a torn / stale message
      arr = col_->arrivals();
      UsedRows used;
      Range tr("eh.master.decode_update");
      const bool decoded = decode(i, arr, used);
      if (!decoded) {
        status = 2;
      } else {
        status = ok ? 0 : 1;
        combine(i, used);
        t_dec = eh::Collector::now();
        t_end = after_combine(i, publish_next);
      }
    }
    return pack(status, arr, i, t_dec, t_end);
  }

  // Host-decoded fallback: coefs[(w, part)] for the given arrivals.
  py::tuple resolve(int i, const std::vector<std::tuple<int, int, double>>& coefs, bool publish_next) {
    std::vector<eh::Arrival> arr = col_->arrivals();
    double t_dec, t_end;
    {
      py::gil_scoped_release nogil;
      UsedRows used;
      for (const auto& [w, p, c] : coefs) push_msg(used, i, w, p, c);
      combine(i, used);
      t_dec = eh::Collector::now();
      t_end = after_combine(i, publish_next);
    }
    return pack(0, arr, i, t_dec, t_end);
  }

  // ---- device-driven rounds (single process, no injected delay) -------------------------
  // Every message is local and finishes with the one gradient launch, so the arrival order
  // (and with it the decode) is fixed before the GPU runs: the collector still decides it,
  // from host probes seen at the round start (ties break by the collector's seeded per-round
  // permutation, exactly like the simultaneous HIP-event probes of begin()).  The host decodes round i and
  // enqueues  grad(i) -> combine_update(i)  while the GPU still runs earlier rounds, so the
  // device never waits for the host between rounds.  With `graph` the whole segment is captured into hipGraphs (at most
  // kGraphRounds rounds each) and replayed with one launch per graph.
  // stamps: int64 GPU [R + 1]; stamps[a] = device time before round a, stamps[i + 1] = start
  // of round i's update (its messages are done).  Returns the arrivals of every round.
  static constexpr int kGraphRounds = 256;

  py::list run_local(int a, int b, bool graph, const Tensor& stamps) {
    need(a >= 0 && a <= b && b <= R_, "round range out of bounds");
    need(remote_.empty() && targets_.empty(), "device-driven rounds need every message local");
    need(n_loc_ > 0 && launcher_ != nullptr, "no local messages");
    need(stamps.is_cuda() && stamps.scalar_type() == at::kLong && stamps.numel() >= R_ + 1, "stamps: int64 [R+1]");
    for (int i = a; i < b; ++i)
      for (int w = 0; w < W_; ++w) need(delays_[static_cast<int64_t>(i) * W_ + w] == 0.0, "injected delay present");
    std::vector<std::vector<eh::Arrival>> arrs;
    std::vector<UsedRows> useds;
    arrs.reserve(b - a);
    useds.reserve(b - a);
    auto decode_round = [&](int i) {
      const double t = eh::Collector::now();
      col_->begin_round(i, t, stop_rule_, k_);
      t_start_[i] = t;
      for (const auto& m : local_) col_->mark_seen(col_->add_host_probe(m.w, m.p, i, 0.0), t);
      need(col_->wait(timeout_), "local arrivals did not satisfy the stop rule");
      UsedRows used;
      need(decode(i, col_->arrivals(), used), "completion pattern missing from the decode table");
      arrs.push_back(col_->arrivals());
      useds.push_back(std::move(used));
      if (drain_) col_->drain(i, timeout_);
    };
    if (graph) {  // a captured segment needs every round decoded before the capture
      Range tr("eh.master.decode_ahead");
      for (int i = a; i < b; ++i) decode_round(i);
    }
    long long* st = reinterpret_cast<long long*>(stamps.data_ptr<int64_t>());
    // The rounds run on the pump's own stream (the legacy default stream cannot be captured),
    // ordered after everything already on the caller's stream and before anything after.
    if (!dev_stream_) {
      dev_stream_ = make_stream();
      join_ev_ = make_event();
    }
    hcheck(hipEventRecord(join_ev_, stream_), "hipEventRecord");
    hcheck(hipStreamWaitEvent(dev_stream_, join_ev_, 0), "hipStreamWaitEvent");
    const hipStream_t caller = stream_;
    stream_ = dev_stream_;  // launcher_/combine() enqueue on stream_
    struct Restore {
      hipStream_t& s;
      hipStream_t v;
      ~Restore() { s = v; }
    } restore{stream_, caller};
    auto enqueue = [&](int i0, int i1) {
      for (int i = i0; i < i1; ++i) {
        // stream mode: decode round i just before enqueueing it, so the host decodes round i + 1
        // while the GPU runs round i (no host-only stretch at the start of a timed segment)
        if (!graph) decode_round(i);
        char* g = ring_slot(G_, g_rows_, i);
        eh::LocalUpdate up;
        if (fused_update_ && prox_.empty() && launcher_->can_fuse_update() &&
            local_update(i, useds[i - a], g, st + i + 1, &up)) {
          hcheck(launcher_->launch_update(beta_row(i), g, up, stream_), "local gradient + update");
          continue;
        }
        hcheck(launcher_->launch(beta_row(i), g, stream_), "local gradient");
        combine(i, useds[i - a], false, st + i + 1);
      }
    };
    Range tr("eh.master.device_rounds");
    hcheck(eh::stamp_launch(st + a, stream_), "stamp");
    if (!graph) {
      enqueue(a, b);
    } else {
      for (int c0 = a; c0 < b; c0 += kGraphRounds) {
        const int c1 = std::min(b, c0 + kGraphRounds);
        hipGraph_t gr = nullptr;
        hipGraphExec_t ex = nullptr;
        hcheck(hipStreamBeginCapture(stream_, hipStreamCaptureModeThreadLocal), "hipStreamBeginCapture");
        try {
          enqueue(c0, c1);
        } catch (...) {
          hipStreamEndCapture(stream_, &gr);
          if (gr) hipGraphDestroy(gr);
          throw;
        }
        hcheck(hipStreamEndCapture(stream_, &gr), "hipStreamEndCapture");
        hcheck(hipGraphInstantiate(&ex, gr, nullptr, nullptr, 0), "hipGraphInstantiate");
        hipGraphDestroy(gr);
        hcheck(hipGraphLaunch(ex, stream_), "hipGraphLaunch");
        graphs_.push_back(ex);
      }
      ++graph_segments_;
    }
    hcheck(hipEventRecord(join_ev_, dev_stream_), "hipEventRecord");
    hcheck(hipStreamWaitEvent(caller, join_ev_, 0), "hipStreamWaitEvent");
    py::list out;
    for (const auto& arr : arrs) {
      py::list lst;
      for (const auto& x : arr) lst.append(py::make_tuple(x.worker, x.part, x.t_rel));
      out.append(lst);
    }
    return out;
  }

  // ---- device-driven rounds with remote workers (csrc/kernels/arbiter.hip) -----------------
  // sources: (host address, device address) of every worker rank's message counter; a remote
  // message belongs to the source with its flag's host address.
  void set_sources(const std::vector<std::pair<uintptr_t, uintptr_t>>& srcs) {
    for (const auto& f : srcs) need(f.first != 0 && f.second != 0, "null source counter");
    arb_src_ = srcs;
    arb_ready_ = false;
  }

  // Why rounds [a, b) cannot run on the device arbiter ("" = they can).
  std::string device_blocker(int a, int b) const {
    if (!prox_.empty()) return "proximal step after the update (L1 penalty)";
    if (blocks_) return "per-model update coefficients (multi-model run)";
    if (comm_) return "messages travel over " + comm_->kind() + " (the arbiter polls IPC counters)";
    if (remote_.empty() || arb_src_.empty()) return "no remote workers";
    if ((int)arb_src_.size() > eh::kArbMaxSrc) return "more than 64 worker ranks";
    if (W_ > eh::kArbMaxW) return "more than 64 workers";
    if ((int)(local_.size() + remote_.size()) > eh::kArbMaxProbes) return "too many message shards";
    if (table_decode(decode_kind_) && W_ > 16) return "decode table too large";
    size_t rows = 0;  // worst case of one decode: every buffer row of every message
    for (const auto& ix : index_) {
      if ((int)ix.size() > eh::kArbMaxRows) return "message with more than 16 shards";
      rows += ix.size();
    }
    if (rows > static_cast<size_t>(eh::kMaxMsgs)) return "more than 128 message rows in a decode";
    for (const auto& m : remote_) {
      bool found = false;
      for (const auto& f : arb_src_) found |= f.first == m.flag;
      if (!found) return "remote message without a source counter";
    }
    for (int i = a; i < b; ++i)
      if (!no_delay(i)) return "injected delays (virtual arrival times live on the host)";
    return "";
  }

  // Enqueue rounds [a, b): the master's own gradient, then one arbiter kernel per round that
  // polls the workers' counters, decides, updates and releases the next beta.  Nothing waits on
  // the host; device_log() reads the rounds back.
  void run_device(int a, int b, double deadline_s) {
    need(a >= 0 && a <= b && b <= R_, "round range out of bounds");
    const std::string why = device_blocker(a, b);
    need(why.empty(), "device-driven rounds: " + why);
    if (!arb_ready_) arb_prepare();
    // a new segment starts clean: no abort from an earlier failed segment (whose failure device_log
    // reports; the engine does not continue a run past it)
    hcheck(hipMemsetAsync(arb_abort_.data_ptr(), 0, sizeof(int), stream_), "hipMemsetAsync(abort)");
    eh::ArbArgs args = arb_args_;
    args.deadline_ticks = static_cast<long long>(std::max(0.001, deadline_s) * stamp_hz());
    long long* tlog = reinterpret_cast<long long*>(arb_tlog_.data_ptr<int64_t>());
    if (a < b && a != prepub_) {  // beta(a) was not released by an earlier arbiter
      put_beta(a);
      hcheck(eh::stamp_launch(tlog + static_cast<int64_t>(a) * eh::kArbLogTicks, stream_), "stamp");
    }
    // Integrity checks ride a side stream: check(i) waits for arbiter i, runs during round i+1's local
    // gradient, and arbiter i+1 waits for it (it fails the round if check(i) found a torn row).
    const bool chk = args.tags != nullptr;
    if (chk && !chk_stream_) {
      chk_stream_ = make_stream();
      arb_ev_ = make_event();
      chk_ev_ = make_event();
    }
    for (int i = a; i < b; ++i) {
      if (n_loc_ > 0 && launcher_) {
        char* g = ring_slot(G_, g_rows_, i);
        for (int k = 0; k < repeat_; ++k) hcheck(launcher_->launch(beta_row(i), g, stream_), "local gradient");
      }
      if (chk && i > a) hcheck(hipStreamWaitEvent(stream_, chk_ev_, 0), "hipStreamWaitEvent");
      hcheck(eh::arbiter_round_launch(args, i, acc_, stream_, chk && i > a), "arbiter_round");
      if (chk) {
        hcheck(hipEventRecord(arb_ev_, stream_), "hipEventRecord");
        hcheck(hipStreamWaitEvent(chk_stream_, arb_ev_, 0), "hipStreamWaitEvent");
        hcheck(eh::arbiter_check_launch(args, i, chk_stream_), "arbiter_check");
        hcheck(hipEventRecord(chk_ev_, chk_stream_), "hipEventRecord");
      }
    }
    if (b > a) {
      if (chk) hcheck(hipStreamWaitEvent(stream_, chk_ev_, 0), "hipStreamWaitEvent");  // device_log sees it
      prepub_ = b;
    }
  }

  // Rounds [a, b) of run_device: (status, arrivals [(worker, part, t_rel)], t_decoded, t_end), times
  // in seconds from the round's beta release.  status 0 ok, 1 timeout, 2 not decodable on the
  // device, 3 skipped after an earlier failure.  Syncs the pump stream.
  py::list device_log(int a, int b) {
    need(arb_ready_, "run_device first");
    hcheck(hipStreamSynchronize(stream_), "hipStreamSynchronize");
    const Tensor lg = arb_log_.cpu(), tl = arb_tlog_.cpu();
    const int* L = lg.data_ptr<int>();
    const int64_t* T = tl.data_ptr<int64_t>();
    const double hz = stamp_hz();
    py::list out;
    for (int i = a; i < b; ++i) {
      const int* l = L + static_cast<int64_t>(i) * eh::kArbLogInts;
      const int64_t* t = T + static_cast<int64_t>(i) * eh::kArbLogTicks;
      py::list arr;
      const int n = std::min(l[1], 2 * eh::kArbMaxW);
      for (int x = 0; x < n && l[0] == 0; ++x)
        arr.append(py::make_tuple(l[4 + 2 * x], l[5 + 2 * x], (t[eh::kArbTickArr + x] - t[0]) / hz));
      std::string why;
      const auto* e = static_cast<const eh::IntegrityErr*>(err_.host);
      if (l[0] == eh::kArbIntegrity || (l[0] == 3 && __atomic_load_n(&e->flag, __ATOMIC_ACQUIRE)))
        why = integrity_message(*e, false);
      // per-round ticks: poll (release of beta(i) -> stop rule), update (stop rule -> combine and
      // checks done), release (-> beta(i+1) released, drain included); seconds
      const double t_stop = l[0] == 0 && n > 0 ? (t[eh::kArbTickArr + n - 1] - t[0]) / hz : -1.0;
      // inside the update: poll joined (all waves past the barrier + acquire), decode done
      const py::tuple sub = py::make_tuple((t[3] - t[0]) / hz, (t[4] - t[0]) / hz);
      out.append(py::make_tuple(l[0], arr, (t[1] - t[0]) / hz, (t[2] - t[0]) / hz, why, t_stop, sub));
    }
    return out;
  }

  // Wall-clock rate of the device timestamps (Hz).
  double stamp_hz() const {
    int khz = 0;
    hcheck(hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, device_), "hipDeviceGetAttribute");
    return 1e3 * khz;
  }
  int graphs_launched() const { return (int)graphs_.size(); }
  // run_local: combine + update inside the slab reduction (default) or as their own launches (A/B, tests)
  void set_fused_update(bool on) { fused_update_ = on; }

  // Update-kernel durations (ms) of every round run so far (host sync).
  std::vector<double> update_ms() {
    hcheck(hipStreamSynchronize(stream_), "hipStreamSynchronize");
    std::vector<double> out(R_, 0.0);
    for (int i = 0; i < R_; ++i) {
      auto& p = upd_ev_[i];
      if (p.first && p.second) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, p.first, p.second) == hipSuccess) out[i] = ms;
      }
    }
    return out;
  }

 private:
  struct Msg {
    int w, p, row;
    uintptr_t flag;
  };

  void check_wp(int w, int p) const { need(w >= 0 && w < W_ && (p == 0 || p == 1), "bad (worker, part)"); }

  void record_t(int i, int which) { record_timed(tev_[i][which], stream_); }

  // Ring slot i % K of a [K, rows, ld] buffer, and row j of beta_in.
  char* ring_slot(const Tensor& X, int rows, int i) const {
    return static_cast<char*>(X.data_ptr()) + static_cast<int64_t>(i % K_) * rows * ld_ * es_;
  }
  char* beta_row(int j) const { return static_cast<char*>(beta_in_.data_ptr()) + static_cast<int64_t>(j) * ld_ * es_; }

  // every buffer row (one per shard) of round i's message (w, p), each with coefficient c
  void push_msg(UsedRows& used, int i, int w, int p, double c) const {
    const auto& ix = index_[2 * w + p];
    if (ix.empty()) throw std::logic_error("message without a buffer");
    for (const auto& [kind, row] : ix) {
      const char* base = kind == 0 ? ring_slot(G_, g_rows_, i) : ring_slot(rbuf_, r_rows_, i);
      used.push_back({base + static_cast<int64_t>(row) * ld_ * es_, c, kind == 0 ? -1 : row});
    }
  }

  // The buffer rows round i's arrivals decode to, in the order of the decoded terms (decode.h).
  bool decode(int i, const std::vector<eh::Arrival>& arr, UsedRows& used) const {
    std::vector<DecodeTerm> terms;
    if (!decode_arrivals(decode_kind_, group_of_, n_groups_, table_, arr, terms)) return false;
    for (const auto& t : terms) push_msg(used, i, t.worker, t.part, t.coef);
    return true;
  }

  // events: time the update with HIP events (host-driven rounds); stamp: device timestamp
  // written by the update kernel at its start (device-driven rounds, graph capture).
  // Round i's combine + update as a LocalUpdate over the G rows of this launch (run_local); false
  // when a decoded row is not one of them.
  bool local_update(int i, const UsedRows& used, const char* g, long long* stamp, eh::LocalUpdate* up) const {
    if ((int)used.size() > eh::kMaxMsgs) return false;
    const int64_t rb = static_cast<int64_t>(ld_) * es_;
    up->nmsg = (int)used.size();
    for (int m = 0; m < up->nmsg; ++m) {
      const int64_t off = static_cast<const char*>(used[m].p) - g;
      if (used[m].row >= 0 || off < 0 || off % rb || off / rb >= launcher_->nslots) return false;
      up->slot[m] = static_cast<int>(off / rb);
      up->coef[m] = used[m].c;
    }
    up->beta = beta_.data_ptr<double>();
    up->u = u_.data_ptr<double>();
    up->hist = hist_.data_ptr<double>() + static_cast<int64_t>(i) * ld_;
    up->beta_w = beta_row(i + 1);
    up->stamp = stamp;
    up->d = d_;
    up->rule = update_rule_;
    up->decay = decay_[i];
    up->gm = gm_[i];
    up->l2 = l2_[i];
    up->theta = theta_[i];
    return true;
  }
  void combine(int i, const UsedRows& used, bool events = true,
               long long* stamp = nullptr) {
    need((int)used.size() <= eh::kMaxMsgs, "too many messages for one combine");
    eh::CombineArgs a{};
    a.nmsg = (int)used.size();
    bool remote = false;
    for (int m = 0; m < a.nmsg; ++m) {
      a.msg[m] = used[m].p;
      a.coef[m] = used[m].c;
      remote |= used[m].row >= 0;
    }
    if (comm_ && remote) {  // order the combine after the receives it reads (their events are complete)
      const int slot = i % K_;
      for (size_t k = 0; k < comm_ranks_.size(); ++k) {
        const auto& [r, row0, n] = comm_ranks_[k];
        bool hit = false;
        for (const auto& u : used) hit |= u.row >= row0 && u.row < row0 + n;
        if (hit) hcheck(hipStreamWaitEvent(stream_, rev_[static_cast<size_t>(slot) * comm_ranks_.size() + k], 0),
                        "hipStreamWaitEvent(recv)");
      }
    }
    if (tags_ && remote) {  // the mailbox rows it reads are checked after the next round starts
      eh::CheckList& cl = check_;
      const int slot = i % K_;
      cl = eh::CheckList{};
      cl.round = i;
      cl.slot = slot;
      cl.es = es_;
      cl.ld = ld_;
      cl.tags = reinterpret_cast<const eh::MsgTag*>(mbox_tags_) + static_cast<int64_t>(slot) * r_rows_;
      for (const auto& u : used)
        if (u.row >= 0) {
          if (cl.n >= eh::kMaxCheckRows) {  // the check list is full: counted, reported by the trainer
            ++check_rows_cut_;
            continue;
          }
          cl.row[cl.n] = u.p;
          cl.mrow[cl.n] = u.row;
          cl.rank[cl.n] = row_rank_[u.row];
          ++cl.n;
        }
      check_pending_ = cl.n > 0;
    }
    auto& ev = upd_ev_[i];
    if (events) {
      if (!ev.second) ev.second = make_event(hipEventDefault);
      record_timed(ev.first, stream_);
    }
    const int nb = blocks_ ? blocks_ : 1;
    const size_t j = static_cast<size_t>(i) * nb;  // round i's coefficients in the per-block schedules
    auto fill = [&](eh::BlockCoefs& bc) {  // the block schedule's, or one block (d_ of ld_ columns)
      if (blocks_)
        eh::set_block_coefs(bc, nb, block_ld_, block_dx_, &bdecay_[j], &bgm_[j], &bl2_[j]);
      else
        eh::set_block_coefs(bc, 1, ld_, d_, &decay_[i], &gm_[i], &l2_[i]);
    };
    if (!prox_.empty()) {  // then the soft threshold
      eh::ProxCoefs pc{};
      fill(pc);
      std::copy_n(&prox_[j], nb, pc.thr);
      hcheck(eh::combine_update_prox_launch(a, acc_, acc_, beta_.data_ptr<double>(), u_.data_ptr<double>(),
                                            hist_.data_ptr<double>() + static_cast<int64_t>(i) * ld_, beta_row(i + 1),
                                            nullptr, pc, theta_[i], update_rule_, stream_, stamp),
             "combine_update_prox");
    } else if (blocks_) {
      eh::BlockCoefs bc{};
      fill(bc);
      hcheck(eh::combine_update_blocks_launch(a, acc_, acc_, beta_.data_ptr<double>(), u_.data_ptr<double>(),
                                              hist_.data_ptr<double>() + static_cast<int64_t>(i) * ld_, beta_row(i + 1),
                                              nullptr, bc, theta_[i], update_rule_, stream_, stamp),
             "combine_update_blocks");
    } else {
      hcheck(eh::combine_update_launch(a, acc_, acc_, beta_.data_ptr<double>(), u_.data_ptr<double>(),
                                       hist_.data_ptr<double>() + static_cast<int64_t>(i) * ld_,
                                       beta_row(i + 1), nullptr, d_, ld_, decay_[i], gm_[i],
                                       l2_[i], theta_[i], update_rule_, stream_, stamp),
             "combine_update");
    }
    if (events) hcheck(hipEventRecord(ev.second, stream_), "hipEventRecord");
  }

  // Device copies of everything the arbiter reads (arbiter.h ArbArgs); built once.
  void arb_prepare() {
    const auto dev = beta_.device();
    auto ints = [&](const std::vector<int>& v) {
      return at::from_blob(const_cast<int*>(v.data()), {(int64_t)v.size()}, at::kInt).clone().to(dev);
    };
    auto dbl = [&](const std::vector<double>& v) {
      return at::from_blob(const_cast<double*>(v.data()), {(int64_t)v.size()}, at::kDouble).clone().to(dev);
    };
    auto u64 = [&](const std::vector<int64_t>& v) {
      return at::from_blob(const_cast<int64_t*>(v.data()), {(int64_t)v.size()}, at::kLong).clone().to(dev);
    };
    std::vector<int> pw, pp, ps;
    for (const auto& m : local_) {  // probe order = begin(): local event probes, then the flag probes
      pw.push_back(m.w);
      pp.push_back(m.p);
      ps.push_back(-1);
    }
    for (const auto& m : remote_) {
      int src = -1;
      for (int j = 0; j < (int)arb_src_.size(); ++j)
        if (arb_src_[j].first == m.flag) src = j;
      pw.push_back(m.w);
      pp.push_back(m.p);
      ps.push_back(src);
    }
    std::vector<int> nsh(2 * W_, 0), nrows(2 * W_, 0), rows(2 * W_ * eh::kArbMaxRows, 0);
    for (int q = 0; q < (int)pw.size(); ++q) ++nsh[2 * pw[q] + pp[q]];
    for (int mi = 0; mi < 2 * W_; ++mi) {
      nrows[mi] = (int)index_[mi].size();
      for (int r = 0; r < nrows[mi]; ++r) rows[mi * eh::kArbMaxRows + r] = (index_[mi][r].first << 24) | index_[mi][r].second;
    }
    const std::vector<int> tie = tie_ranks(col_->tie_seed(), R_, W_);
    const std::vector<double> table = table_decode(decode_kind_) ? flat_table(table_, W_) : std::vector<double>{};
    std::vector<int64_t> src, tgt;
    for (const auto& f : arb_src_) src.push_back(static_cast<int64_t>(f.second));
    for (const auto& t : targets_) {
      tgt.push_back(static_cast<int64_t>(t.first));
      tgt.push_back(static_cast<int64_t>(t.second));
    }
    arb_keep_ = {ints(group_of_), ints(pw), ints(pp), ints(ps), ints(nsh), ints(nrows), ints(rows), ints(tie),
                 dbl(decay_), dbl(gm_), dbl(l2_), dbl(theta_), u64(src.empty() ? std::vector<int64_t>{0} : src),
                 u64(tgt.empty() ? std::vector<int64_t>{0, 0} : tgt),
                 table.empty() ? at::Tensor() : dbl(table),
                 ints(row_rank_.empty() ? std::vector<int>{0} : row_rank_)};
    arb_log_ = at::zeros({static_cast<int64_t>(R_) * eh::kArbLogInts}, at::TensorOptions().dtype(at::kInt).device(dev));
    arb_tlog_ = at::zeros({static_cast<int64_t>(R_) * eh::kArbLogTicks}, at::TensorOptions().dtype(at::kLong).device(dev));
    arb_abort_ = at::zeros({1}, at::TensorOptions().dtype(at::kInt).device(dev));
    eh::ArbArgs g{};
    g.W = W_;
    g.n_groups = n_groups_;
    g.rule = stop_rule_;
    g.k = k_;
    g.decode = decode_kind_;
    g.drain = drain_ ? 1 : 0;
    g.nprobe = (int)pw.size();
    g.nsrc = (int)arb_src_.size();
    g.ntarget = (int)targets_.size();
    g.K = K_;
    g.ld = ld_;
    g.d = d_;
    g.g_rows = g_rows_;
    g.r_rows = r_rows_;
    g.R = R_;
    g.update_rule = update_rule_;
    g.group_of = arb_keep_[0].data_ptr<int>();
    g.probe_w = arb_keep_[1].data_ptr<int>();
    g.probe_p = arb_keep_[2].data_ptr<int>();
    g.probe_src = arb_keep_[3].data_ptr<int>();
    g.nsh = arb_keep_[4].data_ptr<int>();
    g.msg_nrows = arb_keep_[5].data_ptr<int>();
    g.msg_rows = arb_keep_[6].data_ptr<int>();
    g.tie = arb_keep_[7].data_ptr<int>();
    g.decay = arb_keep_[8].data_ptr<double>();
    g.gm = arb_keep_[9].data_ptr<double>();
    g.l2 = arb_keep_[10].data_ptr<double>();
    g.theta = arb_keep_[11].data_ptr<double>();
    g.src_flag = reinterpret_cast<const unsigned long long*>(arb_keep_[12].data_ptr<int64_t>());
    g.targets = reinterpret_cast<const unsigned long long*>(arb_keep_[13].data_ptr<int64_t>());
    g.table = arb_keep_[14].defined() ? arb_keep_[14].data_ptr<double>() : nullptr;
    g.beta = beta_.data_ptr<double>();
    g.u = u_.data_ptr<double>();
    g.hist = hist_.data_ptr<double>();
    g.beta_in = beta_in_.data_ptr();
    g.G = G_.defined() ? G_.data_ptr() : nullptr;
    g.rbuf = rbuf_.defined() ? rbuf_.data_ptr() : nullptr;
    g.log = arb_log_.data_ptr<int>();
    g.tlog = reinterpret_cast<long long*>(arb_tlog_.data_ptr<int64_t>());
    g.abort = arb_abort_.data_ptr<int>();
    g.tags = tags_ ? reinterpret_cast<const eh::MsgTag*>(mbox_tags_) : nullptr;
    g.row_rank = arb_keep_[15].data_ptr<int>();
    g.inbox_tag_off = inbox_tag_off_;
    arb_checks_ = at::zeros({static_cast<int64_t>(2 * sizeof(eh::CheckList))}, at::TensorOptions().dtype(at::kByte).device(dev));
    g.checks = reinterpret_cast<eh::CheckList*>(arb_checks_.data_ptr());
    g.err = static_cast<eh::IntegrityErr*>(err_.dev);
    arb_args_ = g;
    arb_ready_ = true;
  }

  // push beta(j) into every worker inbox (put + signal kernels on the pump stream)
  // one send of beta(j) per worker rank, each on its own stream behind the update that wrote it
  // senders_only: only the ranks that send messages -- the end-of-run beta(R) goes to the WorkerPumps
  // with stale-round skipping (set_skip_stale_comm) and nowhere else: a rank hosting no message runs
  // the Python worker loop, which receives beta(0..R-1) only, and an unmatched send could hold the
  // pump's stream (comm.h: a send blocks until the peer's matching call).
  void put_beta_comm(int j, bool senders_only = false) {
    const void* src = beta_row(j);
    hcheck(hipEventRecord(bev_, stream_), "hipEventRecord(beta)");
    for (int r : comm_peers_) {
      if (senders_only && std::none_of(comm_ranks_.begin(), comm_ranks_.end(),
                                       [r](const auto& c) { return std::get<0>(c) == r && std::get<2>(c) > 0; }))
        continue;
      hcheck(hipStreamWaitEvent(send_st_.at(r), bev_, 0), "hipStreamWaitEvent(beta)");
      comm_->send(r, src, static_cast<int64_t>(ld_) * es_, send_st_.at(r));
    }
  }
  void put_beta(int j) {
    int64_t* rec = rec_.defined() && j <= R_ ? rec_.data_ptr<int64_t>() + 2 * static_cast<int64_t>(j) : nullptr;
    if (rec) hcheck(eh::stamp_launch(reinterpret_cast<long long*>(rec), stream_), "stamp(beta put)");
    put_beta_kernels(j);
    if (rec) hcheck(eh::stamp_launch(reinterpret_cast<long long*>(rec + 1), stream_), "stamp(beta put)");
  }
  // The reference event of device-timed receive events: the sample with the shortest host round trip.
  void calibrate_ref_event() {
    std::vector<Event> evs(8);
    double best = 1e30;
    for (auto& ev : evs) {
      ev = make_event(hipEventDefault);
      const double ta = eh::Collector::now();
      hcheck(hipEventRecord(ev, stream_), "hipEventRecord(ref)");
      hcheck(hipEventSynchronize(ev), "hipEventSynchronize(ref)");
      const double tb = eh::Collector::now();
      if (tb - ta < best) {
        best = tb - ta;
        ref_t_ = 0.5 * (ta + tb);
        std::swap(ref_ev_, ev);  // the ones not picked go with evs
      }
    }
  }
  void put_beta_kernels(int j) {
    if (comm_) {
      if (timing_) record_t(j, 0);
      put_beta_comm(j);
      if (timing_) record_t(j, 1);
      return;
    }
    if (targets_.empty()) return;
    const void* src = beta_row(j);
    if (timing_) record_t(j, 0);
    for (size_t k0 = 0; k0 < targets_.size(); k0 += eh::kMaxPuts) {
      eh::PutArgs a{};
      a.n = 0;
      for (size_t k = k0; k < targets_.size() && a.n < eh::kMaxPuts; ++k) {
        auto& d = a.d[a.n];
        d = eh::PutDesc{src, reinterpret_cast<char*>(targets_[k].first) + static_cast<int64_t>(j) * ld_ * es_,
                        static_cast<long long>(ld_) * es_,
                        reinterpret_cast<unsigned long long*>(targets_[k].second),
                        static_cast<unsigned long long>(j + 1),
                        reinterpret_cast<unsigned int*>(counters_.data_ptr<int>()) + k};
        if (tags_) {
          d.tag = reinterpret_cast<eh::MsgTag*>(reinterpret_cast<char*>(targets_[k].first) + inbox_tag_off_) + j;
          d.csum = reinterpret_cast<unsigned long long*>(csum_.data_ptr<int64_t>()) + a.n * eh::kMaxTagRows;
          d.rows = 1;
          d.es = es_;
          d.rank = 0;
          d.corrupt = sabotage("beta", static_cast<int>(k) + 1, j) ? 1 : 0;
        }
        ++a.n;
      }
      hcheck(eh::put_signal_launch(a, put_blocks(static_cast<long long>(ld_) * es_), stream_), "put_signal(beta)");
    }
    if (timing_) record_t(j, 1);
  }

  // Enqueue the pending check of the last combined round (integrity.h CheckList): off the round's
  // critical path, the rows stay intact until slot reuse K >= 2 rounds later.
  void flush_check() {
    if (!check_pending_) return;
    check_pending_ = false;
    hcheck(eh::check_list_launch(check_, static_cast<eh::IntegrityErr*>(err_.dev), stream_), "check_list");
  }

  // No virtual delay applies in round i: the local messages' entries of the delay table and the remote
  // ones of the remote table (a physically late rank's own lateness is no virtual delay).
  bool no_delay(int i) const {
    const double* dl = delays_.data() + static_cast<int64_t>(i) * W_;
    const double* dr = remote_delays_.empty() ? dl : remote_delays_.data() + static_cast<int64_t>(i) * W_;
    for (const auto& m : local_)
      if (dl[m.w] != 0.0) return false;
    for (const auto& m : remote_)
      if (dr[m.w] != 0.0) return false;
    return true;
  }

  double after_combine(int i, bool publish_next) {
    const bool next = publish_next && i + 1 < R_;
    if (drain_ && next && !drain_flags_.empty() && no_delay(i) && no_delay(i + 1)) {
      // Device-side drain: the pump stream waits until every worker rank's round-i flag is set
      // (hipStreamWaitValue64 on the shared flags), then pushes beta(i+1) — queued now, so the
      // put leaves as soon as the last message lands instead of after a host wake-up + launch.
      // The host drain below still gates the round's bookkeeping (t_start of round i+1).
      for (const auto& f : drain_flags_)
        hcheck(hipStreamWaitValue64(stream_, reinterpret_cast<void*>(f.second), static_cast<uint64_t>(i + 1),
                                    hipStreamWaitValueGte),
               "hipStreamWaitValue64(message flag)");
      put_beta(i + 1);
      prepub_ = i + 1;
      Range tr("eh.master.drain");
      if (!col_->drain(i, timeout_)) {
        // a worker rank is gone: release the queued waits (store the value they wait for) so no
        // wait is left on the GPU; its late message, if any, lands in a slot nobody reads
        for (const auto& f : drain_flags_) {
          auto* h = reinterpret_cast<uint64_t*>(f.first);
          if (__atomic_load_n(h, __ATOMIC_ACQUIRE) < static_cast<uint64_t>(i + 1))
            __atomic_store_n(h, static_cast<uint64_t>(i + 1), __ATOMIC_RELEASE);
        }
      }
    } else if (drain_) {
      Range tr("eh.master.drain");
      col_->drain(i, timeout_);
    }
    const double t_end = eh::Collector::now();
    if (next) begin(i + 1);
    return t_end;
  }

  py::tuple pack(int status, const std::vector<eh::Arrival>& arr, int i, double t_dec, double t_end) const {
    py::list lst;
    for (const auto& a : arr) lst.append(py::make_tuple(a.worker, a.part, a.t_rel));
    return py::make_tuple(status, lst, t_start_[i], t_dec, t_end, t_waited_);
  }

  eh::Collector* col_;
  int W_, R_, K_, d_, ld_, device_;
  double timeout_;
  hipStream_t stream_ = nullptr;
  int acc_ = 0, es_ = 8;
  Tensor beta_, u_, hist_, beta_in_, G_, rbuf_, counters_;
  std::shared_ptr<GradLauncher> launcher_;
  int n_loc_ = 0, g_rows_ = 1, r_rows_ = 1;
  std::vector<Msg> local_, remote_;
  std::vector<std::vector<std::pair<int, int>>> index_;  // [2*w+p] -> (0 local | 1 remote, row) per shard
  std::vector<std::pair<uintptr_t, uintptr_t>> targets_;
  std::vector<std::pair<uintptr_t, uintptr_t>> drain_flags_;
  int prepub_ = -1;  // round whose beta is already queued (device-side drain / the arbiter)
  std::shared_ptr<eh::P2PComm> comm_;                 // stream-ordered p2p (set_comm); null: IPC mailbox
  // device times of physically late ranks (set_device_times) and per-round records (set_records)
  bool dev_times_ = false;
  std::map<int, eh::DeviceClock> clocks_;
  uintptr_t ring_host_ = 0;
  int ring_ = 1;
  Event ref_ev_;
  double ref_t_ = 0.0;
  Tensor rec_;
  std::vector<std::tuple<int, int, int>> comm_ranks_;  // (rank, first mailbox row, rows) of every sender
  std::vector<int> comm_peers_;                        // every worker rank (beta receivers)
  std::vector<Stream> comm_own_;                       // the per-peer streams, each once
  std::map<int, hipStream_t> send_st_, recv_st_;       // per-peer streams (a link stream under both)
  std::vector<Event> rev_;                             // [K][sender] receive-done events (collector probes)
  Event bev_;                                          // beta(j) written (the sends wait on it)
  bool tags_ = false;               // integrity tags on (set_integrity)
  int64_t check_rows_cut_ = 0;      // decoded mailbox rows past a round's check list (kMaxCheckRows): unchecked
  uintptr_t mbox_tags_ = 0;         // device address of the mailbox tag slots [K][r_rows]
  int64_t inbox_tag_off_ = 0;       // worker inbox base -> its tag slots
  std::vector<int> row_rank_;       // [r_rows] sender rank of each mailbox row
  HostMapped err_{sizeof(eh::IntegrityErr)};  // first integrity failure (eh::IntegrityErr)
  Tensor csum_;                     // beta put checksum scratch
  eh::CheckList check_{};           // mailbox rows of the last combined round, checked after the next begins
  bool check_pending_ = false;
  std::vector<std::pair<uintptr_t, uintptr_t>> arb_src_;
  bool arb_ready_ = false;
  eh::ArbArgs arb_args_{};
  std::vector<Tensor> arb_keep_;
  Tensor arb_log_, arb_tlog_, arb_abort_, arb_checks_;
  std::vector<double> decay_, gm_, l2_, theta_, delays_, remote_delays_;
  int blocks_ = 0, block_ld_ = 0, block_dx_ = 0;  // set_block_schedule: per-model coefficients [R * blocks_]
  std::vector<double> bdecay_, bgm_, bl2_;
  std::vector<double> prox_;  // set_prox_schedule: soft thresholds [R * max(1, blocks_)]; empty = no proximal step
  int repeat_ = 1;
  int update_rule_ = 0, stop_rule_ = 0, k_ = 0;
  bool drain_ = false;
  bool skip_ = false;  // drain "lazy": stale-round skipping (set_skip_stale)
  int decode_kind_ = kSumPart0, n_groups_ = 1;
  std::vector<int> group_of_;
  std::map<uint64_t, std::vector<double>> table_;
  std::vector<double> t_start_;
  double t_waited_ = 0.0;  // host time the last wait() returned (phase timing)
  std::vector<std::pair<Event, Event>> upd_ev_;
  std::vector<Event> loc_ev_;
  std::vector<hipGraphExec_t> graphs_;  // device-driven segments (destroyed after a sync)
  Stream dev_stream_;                    // stream of the device-driven rounds (capturable)
  bool fused_update_ = true;              // run_local: combine + update inside the slab reduction
  Stream chk_stream_;                    // run_device: arbiter_check kernels beside the local gradient
  Event arb_ev_, chk_ev_;
  Event join_ev_;
  int graph_segments_ = 0;
  bool timing_ = false;
  std::vector<std::array<Event, 4>> tev_;  // [round] put start/end, gradient start/end
};

}  // namespace

namespace eh {
void bind_master_pump(py::module& m) {
  py::class_<MasterPump>(m, "MasterPump")
      .def(py::init<eh::Collector*, int, int, int, int, int, int, double>(), py::arg("collector"), py::arg("W"),
           py::arg("R"), py::arg("K"), py::arg("d"), py::arg("ld"), py::arg("device"), py::arg("timeout"),
           py::keep_alive<1, 2>())
      .def("set_state", &MasterPump::set_state)
      .def("set_local", &MasterPump::set_local)
      .def("set_remote", &MasterPump::set_remote)
      .def("set_puts", &MasterPump::set_puts)
      .def("set_drain_flags", &MasterPump::set_drain_flags)
      .def("set_remote_delays", &MasterPump::set_remote_delays)
      .def("set_comm", &MasterPump::set_comm, py::arg("comm"), py::arg("ranks"), py::arg("peers"))
      .def_property_readonly("comm_kind", &MasterPump::comm_kind)
      .def("set_repeat", &MasterPump::set_repeat)
      .def("set_skip_stale", &MasterPump::set_skip_stale, py::arg("on"))
      .def_property_readonly("comm_streams", &MasterPump::comm_streams)
      .def("stream_handles", &MasterPump::stream_handles)
      .def("finish_run", &MasterPump::finish_run)
      .def_property_readonly("skipped", &MasterPump::skipped)
      .def_property_readonly("stale_arrivals", &MasterPump::stale_arrivals)
      .def("set_integrity", &MasterPump::set_integrity, py::arg("mbox_tags"), py::arg("inbox_tag_off"), py::arg("on"))
      .def_property_readonly("integrity", &MasterPump::integrity)
      .def("check_integrity", &MasterPump::check_integrity)
      .def("check_rows_cut", &MasterPump::check_rows_cut)
      .def("final_check", &MasterPump::final_check)
      .def("set_sources", &MasterPump::set_sources)
      .def("device_blocker", &MasterPump::device_blocker)
      .def("run_device", &MasterPump::run_device, py::arg("a"), py::arg("b"), py::arg("deadline_s"))
      .def("device_log", &MasterPump::device_log)
      .def("set_schedule", &MasterPump::set_schedule)
      .def("set_block_schedule", &MasterPump::set_block_schedule)
      .def("set_prox_schedule", &MasterPump::set_prox_schedule)
      .def("set_decode", &MasterPump::set_decode)
      .def("add_table", &MasterPump::add_table)
      .def("begin", &MasterPump::begin, py::call_guard<py::gil_scoped_release>())
      .def("finish", &MasterPump::finish)
      .def("resolve", &MasterPump::resolve)
      .def("update_ms", &MasterPump::update_ms)
      .def("run_local", &MasterPump::run_local, py::arg("a"), py::arg("b"), py::arg("graph"), py::arg("stamps"))
      .def("stamp_hz", &MasterPump::stamp_hz)
      .def("set_timing", &MasterPump::set_timing)
      .def("timing_ms", &MasterPump::timing_ms)
      .def("graphs_launched", &MasterPump::graphs_launched)
      .def("set_fused_update", &MasterPump::set_fused_update, py::arg("on"))
      .def("set_device_times", &MasterPump::set_device_times, py::arg("clocks"), py::arg("ring_host"), py::arg("ring"))
      .def("set_records", &MasterPump::set_records, py::arg("on"))
      .def("records", &MasterPump::records)
      .def("probe_log", [](MasterPump& p) { return p.probe_log(); });
}
}  // namespace eh
