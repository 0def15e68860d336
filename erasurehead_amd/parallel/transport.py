"""Message transports between the master (rank 0) and the worker ranks (L7).

The reference moves every vector with mpi4py point-to-point calls: the master "broadcasts"
beta with W Isends (ref src/naive.py:97-98), workers Isend their gradient with tag = round
(ref :150) into pre-posted Irecvs (ref :66-79) and the master Waitany()s on them.  Three
interchangeable transports implement that contract here; the engine never branches on them:

  ``ipc``   MI355X fast path.  Every rank exports a raw device region with
            hipIpcGetMemHandle; beta is *pushed* by the master GPU straight into each
            worker's per-round inbox and gradients are pushed by each worker GPU straight
            into the master's mailbox ring, both with the put+signal kernel
            (csrc/kernels/transport.hip): payload over xGMI, then a 64-bit round counter
            release-stored into shared host memory.  The master's collector polls those
            counters natively (flag probes); workers poll their beta counter.  No RCCL
            kernel, no host copy, one launch per direction per round.
  ``rccl``  native RCCL p2p (csrc/runtime/comm.cpp): a 2-rank communicator per direction per
            pair, ncclSend/ncclRecv on per-peer streams, HIP events behind each receive feed the
            collector; driven by the same native pumps as ``ipc``.
  ``loopback`` the rccl path's exact semantics over IPC staging rings, for ranks sharing a GPU
            (RCCL refuses that): how the single-GPU box tests the RCCL pump code.
  ``rccl-self`` ranks as threads of ONE process on one GPU (parallel/dist.py ThreadEnv): every
            channel is a 1-rank RCCL communicator whose grouped ncclSend + ncclRecv to self moves
            the payload through a staging ring, so the pumps' comm mode executes real RCCL calls
            on the one-GPU box (csrc/runtime/comm.cpp RcclSelfLoop).
  ``gloo``  CPU tensors over gloo (tests, multi-process plumbing without a GPU).

Buffers are per (round mod K) for messages and per round for beta, so a lagging worker can
never see its beta overwritten (the reference's single-buffer race).
"""
from __future__ import annotations

import os
import sys
import time
import uuid
from typing import Dict, List, Optional

import numpy as np
import torch
import torch.distributed as dist

TAG_BYTES = 16  # csrc/kernels/integrity.h MsgTag
TAG_STRIDE = 1024  # gloo tags: beta of round i = 2*i*S, message j of round i = 2*(i*S+j)+1


def _tag_beta(i: int) -> int:
    return 2 * i * TAG_STRIDE


def _tag_msg(i: int, j: int) -> int:
    return 2 * (i * TAG_STRIDE + j) + 1


class Transport:
    """Interface used by engine/trainer.py (see the module docstring)."""

    name = "base"
    fallback_reason: Optional[str] = None  # why the preferred transport was not used (loud fallback)
    pairs: List[dict] = []  # IPC: per worker rank peer-access record (IpcTransport._check_topology)

    def __init__(self, env, R: int, K: int, ld: int, dtype: torch.dtype, n_local: int,
                 remote_counts: Dict[int, int]):
        self.env = env
        self.R, self.K, self.ld, self.dtype = R, K, ld, dtype
        self.n_local = n_local
        self.remote_counts = remote_counts  # master: rank -> number of messages it sends
        self.n_rem = sum(remote_counts.values())
        # master: first mailbox row of every rank's messages (contiguous per rank)
        self.row0: Dict[int, int] = {}
        j = 0
        for r in sorted(remote_counts):
            self.row0[r] = j
            j += remote_counts[r]

    # ---- buffers owned by the transport --------------------------------------------
    def make_rbuf(self) -> torch.Tensor:
        """Master mailbox ring [K, n_rem, ld]."""
        return torch.zeros((self.K, max(1, self.n_rem), self.ld), dtype=self.dtype, device=self.env.device)

    # ---- master side -------------------------------------------------------------------
    def send_beta(self, i: int, beta: torch.Tensor) -> None:
        raise NotImplementedError

    def post_recvs(self, i: int, slot: int, col, rbuf: torch.Tensor, msgs_by_rank, delays,
                   physical: bool = False) -> None:
        """physical: the worker ranks are really late (--delay-on worker): arrival = completion."""
        raise NotImplementedError

    def before_read(self, slot: int, j: int) -> None:
        """Order the current stream after message (slot, j) landed (no-op when the host already knows)."""

    def release_workers(self, value: int) -> None:
        """Master, drain "lazy", after its last round: every worker's beta counter to ``value`` (R + 1),
        so rounds a late worker still has queued are stale and skipped (no-op without counters)."""

    # ---- worker side -------------------------------------------------------------------
    def recv_beta(self, i: int) -> torch.Tensor:
        raise NotImplementedError

    def stale(self, i: int) -> bool:
        """Worker, drain "lazy": beta(i+1) is already out, so round i is stale (only where the transport
        can tell without receiving it: the IPC counters)."""
        return False

    def rounds_done(self, R: int) -> None:
        """Worker, drain "lazy": announce every round < R as put or skipped (the master's final drain)."""

    def send_msgs(self, i: int, G_slot: torch.Tensor) -> None:
        raise NotImplementedError

    def finish(self) -> None:
        """Worker: every send issued so far has completed."""

    def abort(self) -> None:
        """Release every operation still queued on a peer that will never answer (stream-ordered p2p):
        after it, a device synchronisation returns; the transport is unusable."""

    def close(self) -> None:
        pass


# ===================================================================================== gloo
class GlooTransport(Transport):
    name = "gloo"
    _generation = 0  # transports built so far in this process (every rank builds them in the same order)

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self._sends: List[List] = [[] for _ in range(self.K)]
        self.bbuf = torch.zeros((2, self.ld), dtype=self.dtype)
        # Tags of this transport live above every earlier transport's: a send or receive a failed run
        # left pending on the process group (Trainer.run_contained) can never match a later run's.
        GlooTransport._generation += 1
        self.tag0 = 2 * TAG_STRIDE * (self.R + 1) * (GlooTransport._generation - 1)
        if self.tag0 + 2 * TAG_STRIDE * (self.R + 1) >= 2 ** 31:
            GlooTransport._generation, self.tag0 = 1, 0

    def send_beta(self, i, beta):
        for r in range(1, self.env.world):
            self._sends[i % self.K].append(dist.isend(beta, r, tag=self.tag0 + _tag_beta(i)))

    def post_recvs(self, i, slot, col, rbuf, msgs_by_rank, delays, physical=False):
        for r in sorted(msgs_by_rank):
            for jj, m in enumerate(msgs_by_rank[r]):
                j = self.row0[r] + jj
                w = dist.irecv(rbuf[slot, j], r, tag=self.tag0 + _tag_msg(i, jj))
                col.add_work(m.worker, m.part, i, w, delays[m.worker], src=r, physical=physical)

    def recv_beta(self, i):
        slot = i % self.K
        for w in self._sends[slot]:
            w.wait()
        self._sends[slot] = []
        b = self.bbuf[i % 2]
        dist.irecv(b, 0, tag=self.tag0 + _tag_beta(i)).wait()
        self._cur = i
        return b

    def send_msgs(self, i, G_slot):
        self._sends[i % self.K] = [dist.isend(G_slot[j], 0, tag=self.tag0 + _tag_msg(i, j))
                                   for j in range(G_slot.shape[0])]

    def finish(self):
        for lst in self._sends:
            for w in lst:
                w.wait()
        self._sends = [[] for _ in range(self.K)]


# ========================================================================= rccl / loopback
class CommTransport(Transport):
    """Stream-ordered point-to-point messaging through a native communicator (csrc/runtime/comm.h).

    ``rccl``: one 2-rank RCCL communicator per direction per (master, worker) pair, created from
    ncclGetUniqueId ids the master broadcasts over the gloo/RCCL control plane.  The
    native pumps drive it (beta: one send per worker rank on its own stream; messages: one receive
    per worker rank into its mailbox rows with a HIP event behind it, the collector's probe); the
    Python round loop uses the same communicator through ``send`` / ``recv`` bindings.
    ``loopback``: the same semantics through IPC staging rings (RCCL refuses two ranks on one GPU),
    so the single-GPU test box runs exactly the code path the RCCL transport runs on a node.
    Buffers are plain device tensors (mailbox ring [K, n_rem, ld], beta inbox [R+1, ld]).
    """

    DEPTH = 2  # loopback staging slots per channel (messages a sender may run ahead)

    def __init__(self, *a, kind: str = "rccl", **kw):
        super().__init__(*a, **kw)
        from .._ext import native

        self.name = kind
        self.C = C = native()
        env = self.env
        self.dev = env.device.index if env.device.index is not None else torch.cuda.current_device()
        self.es = torch.tensor([], dtype=self.dtype).element_size()
        self.cs = torch.cuda.current_stream(env.device)
        self._regs = []
        self.flags = None
        counts = env.broadcast_object(self.remote_counts, 0)  # every rank: how many rows each rank sends
        if kind == "rccl":
            ids = {r: (C.nccl_unique_id(), C.nccl_unique_id()) for r in range(1, env.world)} if env.is_master else None
            ids = env.broadcast_object(ids, 0)
            if env.is_master:  # out(r): master -> r (master is rank 0 in it); in(r): r -> master
                links = [x for r in range(1, env.world) for x in ((r, "out", ids[r][0], 0), (r, "in", ids[r][1], 1))]
            else:
                r = env.rank
                links = [(0, "in", ids[r][0], 1), (0, "out", ids[r][1], 0)]
            self.comm = C.RcclComm(self.dev, links)
        elif kind == "loopback":
            self.comm = self._loopback(counts)
        elif kind == "rccl-self":  # thread ranks of one process (parallel/dist.py ThreadEnv): RCCL on one GPU
            if env.backend != "threads":
                raise ValueError("the rccl-self transport runs ranks as threads of one process (ThreadEnv)")
            cap = max([self.ld * self.es] + [n * self.ld * self.es for n in counts.values()])
            loop = C.RcclSelfLoop(self.dev, env.world, self.DEPTH, cap) if env.is_master else None
            self.selfloop = env.broadcast_object(loop, 0)
            self.comm = self.selfloop.view(env.rank)
        else:
            raise ValueError(f"unknown communicator {kind!r}")
        env.barrier()
        self.pairs = []
        self._ps: Dict[int, torch.cuda.Stream] = {}  # python round loop's per-peer streams (created on use)
        if env.is_master:
            self.beta_ev = torch.cuda.Event()
            self.rem_ev = [[torch.cuda.Event() for _ in range(max(1, self.n_rem))] for _ in range(self.K)]
            self.ev_of = [list(evs) for evs in self.rem_ev]
        else:
            self.inbox = torch.zeros((self.R + 1, self.ld), dtype=self.dtype, device=env.device)
            self.bev = torch.cuda.Event()
            self.gev = torch.cuda.Event()
            self.send_done: List[Optional[torch.cuda.Event]] = [None] * self.K

    def _loopback(self, counts):
        """Staging rings (receiver-owned IPC regions) + one shared array of 64-bit counters: per worker
        rank r, [4r] beta ready, [4r+1] beta consumed, [4r+2] messages ready, [4r+3] messages consumed.
        A counter lives with the rank that waits on it: the receiver's ready, the sender's consumed."""
        env, C, w = self.env, self.C, self.env.world
        owners = [0] * (4 * w)
        for r in range(1, w):
            owners[4 * r] = owners[4 * r + 3] = r
        bcap = self.ld * self.es
        mcap = {r: max(16, counts.get(r, 0) * self.ld * self.es) for r in range(1, w)}
        if env.is_master:
            name = "/eh_lb_" + uuid.uuid4().hex[:16]
            self.flags = C.ShmFlags(name, 4 * w, True, True, 0, owners)
            own = {r: C.IpcRegion(self.DEPTH * mcap[r], self.dev, True) for r in range(1, w)}  # message rings
            info = (name, {r: reg.handle() for r, reg in own.items()})
        else:
            info = None
        info = env.broadcast_object(info, 0)
        if not env.is_master:
            self.flags = C.ShmFlags(info[0], 4 * w, False, True, env.rank, owners)
            own = {0: C.IpcRegion(self.DEPTH * bcap, self.dev, True)}  # this rank's beta ring
        self._regs += list(own.values())
        handles = env.gather_objects(None if env.is_master else own[0].handle())
        handles = env.broadcast_object(handles, 0)
        f = self.flags

        def ch(peer, direction, ring, cap, k):
            host = [f.host_addr(j) if owners[j] == env.rank else 0 for j in (k, k + 1)]
            return (peer, direction, ring, cap, self.DEPTH, f.dev_addr(k), f.dev_addr(k + 1), host[0], host[1])
        chans = []
        if env.is_master:
            for r in range(1, w):
                peer_ring = C.IpcRegion(handles[r], self.DEPTH * bcap, self.dev)
                self._regs.append(peer_ring)
                chans.append(ch(r, "out", peer_ring.ptr, bcap, 4 * r))
                if counts.get(r, 0):
                    chans.append(ch(r, "in", own[r].ptr, mcap[r], 4 * r + 2))
        else:
            r = env.rank
            ring = C.IpcRegion(info[1][r], self.DEPTH * mcap[r], self.dev)
            self._regs.append(ring)
            chans.append(ch(0, "in", own[0].ptr, bcap, 4 * r))
            if counts.get(r, 0):
                chans.append(ch(0, "out", ring.ptr, mcap[r], 4 * r + 2))
        env.barrier()
        if env.is_master:
            f.unlink()
        return C.LoopbackComm(self.dev, chans)

    @property
    def ps(self) -> Dict[int, torch.cuda.Stream]:
        """Per-peer streams of the Python round loop (the native pumps own theirs)."""
        if not self._ps:
            peers = range(1, self.env.world) if self.env.is_master else [0]
            self._ps = {r: torch.cuda.Stream(self.env.device) for r in peers}
        return self._ps

    # ---- preflight -------------------------------------------------------------------------
    def preflight(self, iters: int = 200, timeout: float = 30.0) -> List[dict]:
        """Collective.  ``iters`` send -> echo round trips of one row between the master and each worker
        rank in turn over THIS communicator (the pumps' own send/recv path), host-timed, every echo
        checked; a wait past ``timeout`` aborts the communicator and raises (never a hang).  Both sides
        issue the same number of operations per channel, so the FIFO pairing of the training rounds
        is unchanged.  Returns one record per worker rank on every rank."""
        env = self.env
        x = torch.zeros(self.ld, dtype=self.dtype, device=env.device)
        y = torch.empty_like(x)
        ev = torch.cuda.Event()

        def wait(what):
            t0 = time.perf_counter()
            while not ev.query():
                if time.perf_counter() - t0 > timeout:
                    self.comm.abort()
                    raise TransportError(f"{self.name} preflight: {what} did not complete within {timeout:.0f}s")
                time.sleep(2e-5)

        recs: Dict[int, dict] = {}
        err = None
        for r in range(1, env.world):
            env.barrier()
            if env.is_master:
                ts, bad = [], 0
                try:
                    for k in range(iters):
                        x.fill_(float(k % 1000) + 0.5)
                        t0 = time.perf_counter()
                        self.comm.send(r, x)
                        self.comm.recv(r, y)
                        ev.record()
                        wait(f"rank 0 <-> rank {r} round trip {k}")
                        ts.append(1e6 * (time.perf_counter() - t0))
                        bad += int(not bool(torch.equal(x, y)))
                except TransportError as e:
                    err = str(e)
                us = np.sort(np.asarray(ts)) if ts else np.zeros(1)
                recs[r] = {"rank": r, "iters": len(ts), "path": self.name,
                           "rtt_clock": "host, send + echo receive complete",
                           "rtt_us_p50": round(float(us[len(us) // 2]), 2),
                           "rtt_us_p99": round(float(us[min(len(us) - 1, int(0.99 * len(us)))]), 2),
                           "payload_errors": bad}
                if bad and err is None:
                    err = f"{self.name} preflight: rank 0 <-> rank {r}: {bad} echoed rows differ"
            elif env.rank == r:
                try:
                    for k in range(iters):
                        self.comm.recv(0, y)
                        self.comm.send(0, y)
                    ev.record()
                    wait(f"rank {r} echo")
                except TransportError as e:
                    err = str(e)
            err = env.broadcast_object(err, 0) if env.is_master else env.broadcast_object(None, 0)
            if err:
                break
        out = env.broadcast_object([recs[r] for r in sorted(recs)] if env.is_master else None, 0)
        env.barrier()
        if err:
            raise TransportError(err)
        return out

    # ---- native pumps --------------------------------------------------------------------
    def check_queue_budget(self, comm_streams: int) -> dict:
        """Master: the pump's comm streams + the compute stream against the hardware queues HIP started
        with (erasurehead_amd/__init__.py); streams beyond them share queues, and a receive parked on a
        straggler would then hold back another worker's.  Warns when over; returns the record."""
        from .. import HW_QUEUES

        need = comm_streams + 1
        if need > HW_QUEUES:
            print(f"[erasurehead] WARNING: {need} streams (comm + compute) > GPU_MAX_HW_QUEUES={HW_QUEUES}: per-peer "
                  "streams share hardware queues, so a straggler's receive can hold back another worker's (set it "
                  "before HIP starts)", file=sys.stderr, flush=True)
        return {"comm_streams": int(comm_streams), "hw_queues": int(HW_QUEUES), "queue_headroom": int(HW_QUEUES - need)}

    def sender_rows(self):
        """(rank, first mailbox row, rows) of every worker rank that sends messages (master)."""
        return [(r, self.row0[r], n) for r, n in sorted(self.remote_counts.items()) if n]

    # ---- master (python round loop) ------------------------------------------------------------
    def send_beta(self, i, beta):
        self.beta_ev.record(self.cs)
        for r in range(1, self.env.world):
            s = self.ps[r]
            s.wait_event(self.beta_ev)
            with torch.cuda.stream(s):
                self.comm.send(r, beta)

    def post_recvs(self, i, slot, col, rbuf, msgs_by_rank, delays, physical=False):
        # one receive per worker rank: its messages are contiguous rows of the mailbox ring and the
        # rank computes (and sends) them together, so they share one completion event
        for r in sorted(msgs_by_rank):
            s = self.ps[r]
            j0, n = self.row0[r], len(msgs_by_rank[r])
            ev = self.rem_ev[slot][j0]
            with torch.cuda.stream(s):
                self.comm.recv(r, rbuf[slot, j0:j0 + n])
                ev.record(s)
            for jj, m in enumerate(msgs_by_rank[r]):
                self.ev_of[slot][j0 + jj] = ev
                col.add_event(m.worker, m.part, i, ev, delays[m.worker], physical)

    def before_read(self, slot, j):
        self.cs.wait_event(self.ev_of[slot][j])

    # ---- worker (python round loop) -----------------------------------------------------------
    def recv_beta(self, i):
        b = self.inbox[i]
        s = self.ps[0]
        with torch.cuda.stream(s):
            self.comm.recv(0, b)
            self.bev.record(s)
        self.cs.wait_event(self.bev)
        slot = i % self.K
        if self.send_done[slot] is not None:  # G[slot] of round i-K has left the GPU
            self.cs.wait_event(self.send_done[slot])
        return b

    def send_msgs(self, i, G_slot):
        slot = i % self.K
        self.gev.record(self.cs)
        s = self.ps[0]
        s.wait_event(self.gev)
        with torch.cuda.stream(s):
            self.comm.send(0, G_slot)  # all of this rank's messages in one send (rows are contiguous)
            ev = self.send_done[slot] or torch.cuda.Event()
            ev.record(s)
            self.send_done[slot] = ev

    def finish(self):
        torch.cuda.synchronize(self.env.device)

    def abort(self):
        if self.comm is not None:
            self.comm.abort()

    def close(self):
        # abort first (a no-op for finished work; a receive or send queued on a dead peer is released),
        # then wait for the device, and only then unmap the staging rings copy kernels may still target
        if self.comm is not None:
            self.comm.abort()
        torch.cuda.synchronize(self.env.device)
        self.comm = None
        for reg in self._regs:
            reg.close()
        self._regs = []
        if self.flags is not None:
            self.flags.close()
            self.flags = None


RcclTransport = CommTransport  # the RCCL p2p transport (kind="rccl")


# ====================================================================================== ipc
class IpcTransport(Transport):
    """HIP IPC mailboxes + put/signal kernels + shared-host round counters.

    Flag layout (one ShmFlags array created by the master; rank r's host polls its beta counter, the
    master's host every other flag): index r (1..world-1) = the
    round counter of beta pushed to rank r (value i+1 <=> beta of round i is in the inbox),
    index world + r = the round counter of rank r's messages in the master mailbox, and from
    ``stamp_base`` on one ring of K landing stamps per rank (two words at stamp_base + 2 (r * K + i % K):
    round i + 1 and when rank r's put of round i landed, on its GPU clock; csrc/runtime/collector.h
    "Device times").
    """

    name = "ipc"
    FINE = True  # mailboxes in fine-grained (coherent) device memory
    HANDSHAKE_TIMEOUT = 30.0  # whole setup handshake, at most (a run's round timeout can shorten it)

    def __init__(self, *a, timeout: float = 600.0, **kw):
        super().__init__(*a, **kw)
        from .._ext import native

        self.C = C = native()
        env = self.env
        self.timeout = timeout
        self.HANDSHAKE_TIMEOUT = min(self.HANDSHAKE_TIMEOUT, max(5.0, float(timeout)))  # 5..30 s
        self.dev = env.device.index if env.device.index is not None else torch.cuda.current_device()
        self.es = torch.tensor([], dtype=self.dtype).element_size()
        dname = {torch.float64: "float64", torch.float32: "float32"}[self.dtype]
        self.dname = dname
        self.counters = torch.zeros(64, dtype=torch.int32, device=env.device)
        self._imports = []
        self.pairs = self._check_topology()  # collective; raises TransportError naming the pairs
        # Every step is attempted on every rank and the verdict is collective, so a failure
        # on one rank (e.g. hipIpcOpenMemHandle between two GPUs) never strands the others
        # inside a collective.
        err: List[str] = []

        def attempt(fn):
            if err:
                return None
            try:
                return fn()
            except Exception as e:  # noqa: BLE001 - reported collectively below
                err.append(f"rank {env.rank}: {type(e).__name__}: {e}")
                return None

        # every region ends with 16-byte integrity tags, one per payload row (csrc/kernels/integrity.h)
        self.inbox_tag_off = (self.R + 1) * self.ld * self.es
        ibytes = self.inbox_tag_off + (self.R + 1) * TAG_BYTES
        self.stamp_base = 2 * env.world + 1
        nflags = self.stamp_base + 2 * env.world * self.K
        owners = [r if 1 <= r < env.world else 0 for r in range(nflags)]
        if env.is_master:
            name = "/eh_" + uuid.uuid4().hex[:16]
            rbytes = self.K * max(1, self.n_rem) * (self.ld * self.es + TAG_BYTES)

            def _mk():
                self.flags = C.ShmFlags(name, nflags, True, True, 0, owners)
                self.rreg = C.IpcRegion(rbytes, self.dev, self.FINE)
                return (name, self.rreg.handle(), rbytes)

            info = attempt(_mk)
        else:
            info = None
        info = env.broadcast_object(info, 0)
        mine = None
        if not env.is_master:
            if info is None:
                err.append("master failed to create the mailbox")

            def _open():
                name, h, rbytes = info
                self.flags = C.ShmFlags(name, nflags, False, True, env.rank, owners)
                self.rremote = C.IpcRegion(h, rbytes, self.dev)
                self._imports.append(self.rremote)
                self.inbox_reg = C.IpcRegion(ibytes, self.dev, self.FINE)
                self.inbox = self.inbox_reg.view(self.dname, [self.R + 1, self.ld], 0)
                return self.inbox_reg.handle()

            mine = attempt(_open)
        allh = env.gather_objects(mine)
        row0, n_rem = env.broadcast_object((self.row0, self.n_rem), 0)
        self.my_row0 = row0.get(env.rank, 0)
        self.mbox_rows = max(1, n_rem)  # rows per slot of the master's mailbox ring
        self.mbox_tag_off = self.K * self.mbox_rows * self.ld * self.es  # tags [K][mbox_rows] after the rows
        if env.is_master:
            self.inbox_remote = {}

            def _import():
                for r in range(1, env.world):
                    if allh[r] is None:
                        raise TransportError(f"rank {r} could not create its inbox")
                    reg = C.IpcRegion(allh[r], ibytes, self.dev)
                    self._imports.append(reg)
                    self.inbox_remote[r] = reg.view(self.dname, [self.R + 1, self.ld], 0)

            attempt(_import)
        errs = env.gather_objects(err[0] if err else None)
        bad = [e for e in errs if e] if env.is_master else None
        bad = env.broadcast_object(bad, 0)
        if bad:
            self.close()
            raise TransportError("IPC mailbox setup failed: " + "; ".join(bad))
        env.barrier()
        if env.is_master:
            self.flags.unlink()  # every rank has it mapped now
        self._verify()

    def _check_topology(self) -> List[dict]:
        """Peer access between the master GPU and every worker GPU, checked per pair BEFORE any
        IPC handle is opened: ranks exchange PCI bus ids (device indices need not agree across
        processes), each side asks hipDeviceCanAccessPeer for its direction.  Returns one record
        per worker rank: {rank, bus, master_bus, same_gpu, master_to_rank, rank_to_master}
        (None = the peer GPU is not visible to that process: the handshake decides)."""
        env, C = self.env, self.C
        mine = (env.rank, self.dev, C.pci_bus_id(self.dev))
        allv = env.broadcast_object(env.gather_objects(mine), 0)
        mbus = allv[0][2]
        rec = None
        if not env.is_master:
            md = C.device_by_pci(mbus)
            rec = {"rank": env.rank, "bus": mine[2], "master_bus": mbus, "same_gpu": mine[2] == mbus,
                   "rank_to_master": C.can_access_peer(self.dev, md) if md >= 0 else None}
        recs = env.gather_objects(rec)
        pairs: List[dict] = []
        if env.is_master:
            for r in range(1, env.world):
                x = dict(recs[r])
                rd = C.device_by_pci(x["bus"])
                x["master_to_rank"] = C.can_access_peer(self.dev, rd) if rd >= 0 else None
                pairs.append(x)
        pairs = env.broadcast_object(pairs, 0)
        bad = [x for x in pairs if x["master_to_rank"] is False or x["rank_to_master"] is False]
        if bad:
            raise TransportError("IPC mailbox needs peer access between the master GPU and every worker GPU; "
                                 "missing for: " + "; ".join(
                                     f"rank {x['rank']} ({x['bus']}) <-> rank 0 ({x['master_bus']}): "
                                     f"master->rank {x['master_to_rank']}, rank->master {x['rank_to_master']}"
                                     for x in bad))
        return pairs

    def mbox_tags_addr(self) -> int:
        """Device address (in this process) of the master mailbox's tag slots [K][mbox_rows]."""
        reg = self.rreg if self.env.is_master else self.rremote
        return reg.ptr + self.mbox_tag_off

    def inbox_tags_addr(self) -> int:
        """Worker: device address of its own inbox's tag slots [R + 1]."""
        return self.inbox_reg.ptr + self.inbox_tag_off

    def make_rbuf(self):
        if not self.env.is_master:
            return torch.zeros((1, 1, self.ld), dtype=self.dtype, device=self.env.device)
        return self.rreg.view(self.dname, [self.K, max(1, self.n_rem), self.ld], 0)

    # ---- setup handshake: every mailbox direction carries a known pattern once ---------
    def _verify(self):
        """Push a pattern both ways through the real put/signal path before training.

        Catches a platform where IPC mappings or the pinned host flags do not work between
        two GPUs: the engine refuses to start (or, with transport='auto', falls back to
        RCCL) instead of training on garbage.
        """
        env = self.env
        errs: List[str] = []
        if env.is_master:
            pat = torch.arange(self.ld, dtype=self.dtype, device=env.device) + 0.5
            puts = [(pat, self.inbox_remote[r][self.R], self.flags.dev_addr(r), 1) for r in range(1, env.world)]
            for k in range(0, len(puts), 16):
                self.C.put_signal(puts[k:k + 16], self.counters)
            torch.cuda.synchronize(env.device)
            rbuf = self.make_rbuf()
            deadline = time.monotonic() + self.HANDSHAKE_TIMEOUT
            for r in range(1, env.world):
                if not self.flags.wait_ge(env.world + r, 1, max(0.0, deadline - time.monotonic())):
                    errs.append(f"rank {r} -> rank 0: message flag never signalled within {self.HANDSHAKE_TIMEOUT:.0f}s "
                                f"(step: worker put+signal into the master mailbox)")
                    continue
                n = self.remote_counts.get(r, 0)
                if n:
                    got = rbuf[0, self.row0[r]:self.row0[r] + n]
                    want = pat.unsqueeze(0) * (r + 1)
                    if not bool(torch.equal(got, want.expand_as(got))):
                        errs.append(f"rank {r} -> rank 0: payload in mailbox rows {self.row0[r]}..{self.row0[r] + n - 1} "
                                    f"differs from the pattern sent (step: worker put over xGMI)")
            for r in range(1, env.world):
                self.flags.store(env.world + r, 0)
                self.flags.store(r, 0)
        else:
            r = env.rank
            if self.flags.wait_ge(r, 1, self.HANDSHAKE_TIMEOUT):
                pat = torch.arange(self.ld, dtype=self.dtype, device=env.device) + 0.5
                if not bool(torch.equal(self.inbox[self.R], pat)):
                    errs.append(f"rank 0 -> rank {r}: beta payload in the inbox differs from the pattern sent "
                                f"(step: master put over xGMI)")
                n = self.n_local
                if os.environ.get("ERASUREHEAD_SABOTAGE") == f"handshake:{r}":  # test hook: this rank never answers
                    pass
                elif n:
                    src = (pat * (r + 1)).unsqueeze(0).repeat(n, 1).contiguous()
                    dst = self.rremote.view(self.dname, [n, self.ld], self.my_row0 * self.ld * self.es)
                    self.C.put_signal([(src, dst, self.flags.dev_addr(env.world + r), 1)], self.counters)
                else:
                    self.C.signal(self.flags.dev_addr(env.world + r), 1, self.dev)
                torch.cuda.synchronize(env.device)
            else:
                errs.append(f"rank 0 -> rank {r}: beta flag never signalled within {self.HANDSHAKE_TIMEOUT:.0f}s "
                            f"(step: master put+signal into the worker inbox)")
        env.barrier()  # master resets the flags only after everyone saw its pattern
        allerr = env.gather_objects(errs)
        allerr = env.broadcast_object([e for es in allerr for e in es] if env.is_master else None, 0)
        if allerr:
            self.close()
            raise TransportError("IPC mailbox handshake failed: " + "; ".join(allerr))
        if env.is_master:
            rbuf = self.make_rbuf()
            rbuf.zero_()
            torch.cuda.synchronize(env.device)
        env.barrier()

    # ---- per-pair preflight (bench.py --gpus N > 1: the first real multi-GPU run checks itself) --
    def preflight(self, iters: int = 1000, timeout: float = 30.0) -> Optional[List[dict]]:
        """Collective.  ``iters`` put -> flag round trips between the master and each worker rank in
        turn, on the device over the real put+signal path (csrc/kernels/transport.hip ping_pong): the
        master block writes pattern k into the worker's spare inbox row and release-stores its counter;
        the worker block checks the row, echoes it into the master's mailbox row and release-stores
        its own counter; the master times counter store -> echo seen and checks the echo.  Returns
        (on every rank) one record per worker rank: round-trip percentiles (device clock), payload
        words that differed in each direction, and the peer-access facts of the pair.  Counters are
        reset to 0 before and after each pair; every wait has a deadline (``timeout``)."""
        env, C, w, R = self.env, self.C, self.env.world, self.R
        words = self.ld * self.es // 8
        dev = env.device.index if env.device.index is not None else torch.cuda.current_device()
        results: Dict[int, dict] = {}
        rbuf = self.make_rbuf() if env.is_master else None
        for r in range(1, w):
            if env.is_master:
                self.flags.store(r, 0)
                self.flags.store(w + r, 0)
            env.barrier()
            if env.is_master:
                echo = self.remote_counts.get(r, 0) > 0
                res = C.ping_pong(self.inbox_remote[r][R].data_ptr(), rbuf[0, self.row0[r]].data_ptr() if echo else 0,
                                  words, words if echo else 0, self.flags.dev_addr(r), self.flags.dev_addr(w + r),
                                  iters, float(timeout), True, dev)
                results[r] = res
            elif env.rank == r:
                out = (self.rremote.view(self.dname, [self.ld], self.my_row0 * self.ld * self.es).data_ptr()
                       if self.n_local else 0)
                res = C.ping_pong(out, self.inbox[R].data_ptr(), words if self.n_local else 0, words,
                                  self.flags.dev_addr(w + r), self.flags.dev_addr(r), iters, float(timeout), False, dev)
                results[r] = res
            env.barrier()
        mine = {r: {"errors": int(v["payload_errors"]), "timeout": bool(v["timeout"]),
                    "rtt": (v["rtt_us"].numpy().tolist() if "rtt_us" in v else None)} for r, v in results.items()}
        if os.environ.get("ERASUREHEAD_SABOTAGE") == f"preflight:{env.rank}" and env.rank in mine:
            mine[env.rank]["errors"] += 1  # test hook: this worker reports one bad payload word (the verdict path)
        got = env.gather_objects(mine)
        env.barrier()
        out, err = None, None
        if env.is_master:
            for r in range(1, w):
                self.flags.store(r, 0)
                self.flags.store(w + r, 0)
            rbuf.zero_()
            torch.cuda.synchronize(env.device)
            out = []
            for p in self.pairs:
                r = p["rank"]
                m, wk = got[0][r], got[r][r]
                if m["timeout"] or wk["timeout"]:
                    err = (f"preflight: rank 0 <-> rank {r}: a put or its echo never signalled "
                           f"within {timeout:.0f}s (device ping-pong)")
                    break
                if wk["errors"] or m["errors"]:
                    err = (f"preflight: rank 0 <-> rank {r}: {wk['errors']} payload words wrong master -> rank, "
                           f"{m['errors']} rank -> master after the counter was seen (device ping-pong)")
                    break
                us = np.sort(np.asarray(m["rtt"]))
                out.append({"rank": r, "iters": iters, "same_gpu": p["same_gpu"],
                            "master_to_rank_peer": p["master_to_rank"], "rank_to_master_peer": p["rank_to_master"],
                            "mailbox": "fine-grained device memory, pinned host counters" if self.FINE else "coarse",
                            "rtt_clock": "device wall clock, counter store -> echo counter seen",
                            "rtt_us_p50": round(float(us[len(us) // 2]), 2),
                            "rtt_us_p99": round(float(us[min(len(us) - 1, int(0.99 * len(us)))]), 2),
                            "rtt_us_max": round(float(us[-1]), 2),
                            "payload_errors_master_to_rank": int(wk["errors"]),
                            "payload_errors_rank_to_master": int(m["errors"])})
        # the verdict is collective: every rank raises the same error (bench.py then rebuilds on RCCL)
        out, err = env.broadcast_object((out, err), 0)
        env.barrier()
        if err is not None:
            raise TransportError(err)
        return out

    # ---- master ------------------------------------------------------------------------
    def send_beta(self, i, beta):
        puts = [(beta, self.inbox_remote[r][i], self.flags.dev_addr(r), i + 1) for r in range(1, self.env.world)]
        for k in range(0, len(puts), 16):
            self.C.put_signal(puts[k:k + 16], self.counters[16 * (k // 16):])

    def post_recvs(self, i, slot, col, rbuf, msgs_by_rank, delays, physical=False):
        w = self.env.world
        for r in sorted(msgs_by_rank):
            addr = self.flags.host_addr(w + r)
            for m in msgs_by_rank[r]:
                col.add_flag(m.worker, m.part, i, addr, i + 1, delays[m.worker], physical)

    def release_workers(self, value):
        for r in range(1, self.env.world):  # stream-ordered behind the last beta put
            self.C.signal(self.flags.dev_addr(r), int(value), self.dev)

    # ---- worker ------------------------------------------------------------------------
    def recv_beta(self, i):
        if not self.flags.wait_ge(self.env.rank, i + 1, self.timeout):
            raise TimeoutError(f"rank {self.env.rank}: no beta for round {i} within {self.timeout}s")
        return self.inbox[i]

    def stale(self, i):
        return self.flags.load(self.env.rank) >= i + 2

    def rounds_done(self, R):
        self.C.signal(self.flags.dev_addr(self.env.world + self.env.rank), int(R), self.dev)

    def send_msgs(self, i, G_slot):
        slot = i % self.K
        n = G_slot.shape[0]
        off = (slot * self.mbox_rows + self.my_row0) * self.ld * self.es
        dst = self.rremote.view(self.dname, [n, self.ld], off)
        self.C.put_signal([(G_slot, dst, self.flags.dev_addr(self.env.world + self.env.rank), i + 1)],
                          self.counters)

    def finish(self):
        torch.cuda.synchronize(self.env.device)

    def close(self):
        for reg in self._imports:
            reg.close()
        self._imports = []
        for attr in ("inbox_reg", "rreg"):
            reg = getattr(self, attr, None)
            if reg is not None:
                reg.close()
        f = getattr(self, "flags", None)
        if f is not None:
            f.close()


class TransportError(RuntimeError):
    pass


def rccl_p2p_preflight(env, ld: int, dtype, iters: int = 200, warm: int = 10) -> Dict[int, dict]:
    """Collective (ranks with their own GPUs, world process group on RCCL): ``iters`` send -> echo
    round trips of one row between the master and each worker rank in turn through
    torch.distributed send/recv, i.e. RCCL point-to-point over xGMI -- the fallback transport's wire
    path, measured beside the IPC mailbox's.  Host-timed (launch + completion), first ``warm`` trips
    (lazy channel setup) dropped.  Returns {rank: {rtt_us_p50, rtt_us_p99, payload_errors}} on the
    master, {} elsewhere."""
    import datetime

    out: Dict[int, dict] = {}
    x = torch.zeros(ld, dtype=dtype, device=env.device)
    y = torch.empty_like(x)
    limit = datetime.timedelta(seconds=30)  # every transfer waits with a deadline: no silent hang
    for r in range(1, env.world):
        env.barrier()
        if env.is_master:
            ts, bad = [], 0
            for k in range(warm + iters):
                x.fill_(float(k % 1000) + 0.5)
                torch.cuda.synchronize(env.device)
                t0 = time.perf_counter()
                dist.isend(x, dst=r).wait(limit)
                dist.irecv(y, src=r).wait(limit)
                torch.cuda.synchronize(env.device)
                if k >= warm:
                    ts.append(1e6 * (time.perf_counter() - t0))
                    bad += int(not bool(torch.equal(x, y)))
            us = np.sort(np.asarray(ts))
            out[r] = {"rccl_rtt_us_p50": round(float(us[len(us) // 2]), 2),
                      "rccl_rtt_us_p99": round(float(us[min(len(us) - 1, int(0.99 * len(us)))]), 2),
                      "rccl_payload_errors": bad}
        elif env.rank == r:
            for _ in range(warm + iters):
                dist.irecv(y, src=0).wait(limit)
                dist.isend(y, dst=0).wait(limit)
            torch.cuda.synchronize(env.device)
        env.barrier()
    return out


def make_transport(kind: str, env, R: int, K: int, ld: int, dtype, n_local: int, remote_counts,
                   timeout: float = 600.0) -> Transport:
    """kind: auto | ipc | rccl | gloo.  auto = gloo on CPU; on GPUs the IPC mailbox after a
    successful handshake, otherwise RCCL (the choice is collective: every rank agrees)."""
    args = (env, R, K, ld, dtype, n_local, remote_counts)
    if kind == "auto":
        kind = os.environ.get("ERASUREHEAD_TRANSPORT", "auto")
    if env.gpu and env.backend == "gloo" and kind == "rccl":
        raise ValueError("ranks share a GPU (RCCL refuses that): use transport ipc, or loopback for the RCCL code path")
    if not env.gpu:
        if kind not in ("auto", "gloo"):
            raise ValueError(f"transport {kind!r} needs GPUs")
        return GlooTransport(*args)
    if kind == "gloo":
        raise ValueError("gloo transport is the CPU path; GPU ranks use ipc or rccl")
    if kind in ("rccl", "loopback", "rccl-self"):
        return CommTransport(*args, kind=kind)
    local_world = int(os.environ.get("LOCAL_WORLD_SIZE", str(env.world)))
    if kind == "auto" and local_world < env.world and env.backend != "gloo":
        return CommTransport(*args, kind="rccl")  # multi-node (torchrun --nnodes > 1): IPC mailboxes are node-local
    if kind in ("ipc", "auto"):
        try:
            return IpcTransport(*args, timeout=timeout)
        except TransportError as e:
            if kind == "ipc" or env.backend == "gloo":
                raise
            if os.environ.get("ERASUREHEAD_NO_FALLBACK"):
                raise TransportError(f"{e} (ERASUREHEAD_NO_FALLBACK set: not falling back to RCCL)") from e
            # loud, recorded degradation: RCCL p2p under the same native pumps (per-round host wake-ups
            # instead of device-side counters); bench.py reports transport + reason per rank
            if env.is_master:
                print("[erasurehead] WARNING: " + str(e) + "\n[erasurehead] WARNING: falling back to RCCL p2p "
                      "(set ERASUREHEAD_NO_FALLBACK=1 or --transport ipc to fail instead)", file=sys.stderr, flush=True)
            tx = CommTransport(*args, kind="rccl")
            tx.fallback_reason = str(e)
            return tx
    raise ValueError(f"unknown transport {kind!r}")
