"""Multi-GPU communicator: one process per MI355X under torch.distributed.

The reference shards sources over MPI ranks with mpi4py and moves N^3 float64 grids through host
memory (pyc2ray/evolve.py:433-437,480-497).  The path has exactly one real exchange step per outer
iteration -- the sum of the per-rank photo-ionisation rate grids -- so that is the only collective
here: an all-reduce (backend "nccl" == RCCL over xGMI) applied IN PLACE to the device-resident
phi_ion grid.  With the "gloo" backend (CPU tests) the grid is staged through the host.

``TorchComm.raytrace_and_allreduce`` optionally PIPELINES that all-reduce with the raytrace
(``PYC2RAY_AMD_OVERLAP=1`` or ``TorchComm(overlap=True)``): with a rank's sources sorted by their first
coordinate and traced in chunks, the planes of the rate grid that later chunks can no longer reach are final
on every rank, so their sum over ranks runs on a second stream while the next chunk is being traced; only the
planes the last chunks touch are summed after the trace.

``TorchComm`` also offers the handful of mpi4py-style methods the reference's evolve3D_MPI calls
(Get_rank, Get_size, Reduce, Bcast, Allreduce, Barrier), and ``MPI`` the constants it reads, so
reference-style driver code can pass ``use_mpi=dist.MPI, comm=dist.TorchComm()``.
"""
import collections
import contextlib
import os
import time

import numpy as np

from . import _capi

__all__ = ["MPI", "TorchComm", "SlabPlan", "init_process_group_from_env"]


class _MPIShim:
    """The attributes of mpi4py.MPI that pyc2ray/evolve.py touches."""
    IN_PLACE = "IN_PLACE"
    DOUBLE = "DOUBLE"
    INT = "INT"
    SUM = "SUM"

    @property
    def COMM_WORLD(self):
        return TorchComm()


MPI = _MPIShim()


def init_process_group_from_env(backend=None):
    """Initialise torch.distributed from RANK / WORLD_SIZE / LOCAL_RANK / MASTER_* (torchrun).
    Returns (rank, world_size, local_rank).  Backend defaults to nccl when a GPU is visible."""
    # the host driver of these machines only supports dmabuf IPC: without this, RCCL's buffer registration across
    # processes fails with "hipIpcGetMemHandle: invalid argument"
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    import torch
    import torch.distributed as dist
    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if backend is None:
        backend = "nccl" if torch.cuda.is_available() else "gloo"
    if not dist.is_initialized():
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29511")
        if backend == "nccl":
            torch.cuda.set_device(local_rank)
        # a collective that never completes aborts the job after this long instead of the backend's default of ten minutes
        # and more (PYC2RAY_AMD_DIST_TIMEOUT_S)
        import datetime
        timeout = datetime.timedelta(seconds=float(os.environ.get("PYC2RAY_AMD_DIST_TIMEOUT_S", "300")))
        dist.init_process_group(backend=backend, rank=rank, world_size=world, timeout=timeout)
    return rank, world, local_rank


def _runs_of(mask):
    """Maximal runs of True in a boolean vector as [(begin, end)), ...]."""
    m = np.concatenate(([False], np.asarray(mask, dtype=bool), [False]))
    edges = np.flatnonzero(m[1:] != m[:-1])
    return [(int(a), int(b)) for a, b in zip(edges[0::2], edges[1::2])]


class SlabPlan:
    """Which planes of the grids travel between which ranks in one outer iteration of a multi-GPU step.

    The rate grid is a sum over sources and the sources are sharded (pyc2ray/evolve.py:360-371), so the reference
    sums N^3 grids over ranks every iteration (Reduce + Bcast, evolve.py:433-437) and broadcasts two more after
    the chemistry (evolve.py:480-481).  A source at plane i0 only rates the planes i0-R..i0+R.  With the source list
    ordered by the first coordinate before it is cut into the reference's contiguous blocks, rank r's rates are
    non-zero only on `reach[r]` = the planes within R of its slab of sources.  So:

      * the chemistry of plane i is done by ONE rank, the owner of the slab own[q] = [q N/P, (q+1) N/P) it lies in;
      * exchange 1 (rates): rank r sends the part of reach[r] inside own[q] to q, for every q != r where that is
        not empty; q adds what it receives, in rank order, to its own contribution: the summed rates of own[q];
      * slab chemistry on own[q] (1/P of the grid per rank instead of all of it on every rank);
      * exchange 2 (ionised fraction): the same runs travel back -- q sends the new xh_av of reach[r] & own[q] to r,
        which needs it to form nHI for its next raytrace;
      * the three convergence scalars are summed over ranks in rank order (identical on every rank).

    Planes travel as contiguous runs (plane i is N*N consecutive doubles of the [i][j][k] grid); for a pair (r, q)
    these are the maximal runs of reach[r] inside own[q], runs closer than MERGE_GAP planes joined (zeros in between are
    harmless, every run is a message) -- usually one, two when r's sources reach q's slab from both sides around the
    periodic box (two ranks: always).  At 256^3, R = 32, 8 ranks with evenly spread sources a rank sends and receives
    2 x 32 planes per exchange (2 x 16.8 MiB in, the same out, to and from its two neighbours over their direct xGMI
    links) instead of taking part in a ring all-reduce of 128 MiB (224 MiB in and out per rank), and runs 1/8 of the
    chemistry.  With R >= N/2 every rank reaches every plane and the scheme degenerates into reduce-scatter +
    all-gather by direct sends.

    Overlap (``send_schedule``): a rank traces its sources -- ordered by first coordinate -- in K chunks; a foreign plane
    that no LATER chunk can reach is final, is folded and sent at once, while the next chunk is being traced.  Which
    planes go after which chunk is again a function of the plan only, so the receiver posts the matching receives
    without being told.

    Everything here is a function of (N, P, R, first coordinates of the sorted sources) only, so every rank derives
    the same plan without communicating."""

    #: runs of reached planes closer than this are sent as one run
    MERGE_GAP = 4

    def __init__(self, N, nprocs, R, shard_i0):
        """shard_i0[r]: 0-based first coordinates of the sources of rank r, in the order they are uploaded (ascending
        when the chunked schedule is used)."""
        self.N, self.P = int(N), int(nprocs)
        N, P = self.N, self.P
        self.own = [(q * N // P, (q + 1) * N // P) for q in range(P)]
        m = int(np.floor(R)) if np.isfinite(R) else N
        self._lo, self._hi = min(m, N // 2), min(m, N // 2 - 1 + N % 2)          # the periodic window, raytracing.cu:122-123
        self.i0 = [np.asarray(shard_i0[r], dtype=np.int64) for r in range(P)]
        self.reach = [self._reach_of(self.i0[r]) for r in range(P)]
        # runs[r][q]: runs of planes rank r contributes to (and needs back from) the slab of rank q
        self.runs = [[[] for _ in range(P)] for _ in range(P)]
        for r in range(P):
            for q in range(P):
                a, b = self.own[q]
                merged = []
                for s0, s1 in _runs_of(self.reach[r][a:b]):
                    if merged and s0 - merged[-1][1] < self.MERGE_GAP:
                        merged[-1] = (merged[-1][0], s1)
                    else:
                        merged.append((s0, s1))
                self.runs[r][q] = [(a + s0, a + s1) for s0, s1 in merged]
        # memos of the schedules below: an iteration must not pay for them again
        self._send_cache, self._recv_cache, self._work_cache, self._back_cache = {}, {}, {}, {}

    def _reach_of(self, i0):
        """Planes the sources at first coordinates i0 can rate."""
        mask = np.zeros(self.N, dtype=bool)
        i0 = np.unique(np.asarray(i0, dtype=np.int64))
        if i0.size:
            if self._lo + self._hi + 1 >= self.N:
                mask[:] = True
            else:
                for d in range(-self._lo, self._hi + 1):
                    mask[(i0 + d) % self.N] = True
        return mask

    def common_chunks(self, K):
        """The chunk count every rank uses: K when every rank's sources are in ascending order of their first coordinate
        (a rank with fewer sources than chunks simply has empty chunks), else 1 -- nothing is final before the end then."""
        if any(np.any(np.diff(i0) < 0) for i0 in self.i0):
            return 1
        return max(1, int(K))

    @staticmethod
    def chunk_bounds(n, K):
        """Rank-local source ranges [b[c], b[c+1]) of the K trace chunks (equal counts, upload order)."""
        return [c * n // K for c in range(K + 1)]

    def send_schedule(self, r, K):
        """sched[c] = [(q, a, b), ...]: the pieces of runs[r][q] (q != r) rank r sends once it has traced its chunks
        0..c -- the planes no later chunk reaches, not sent before; the last chunk sends everything that is left.  Every
        plane of every run is sent exactly once.  (Memoised: an iteration must not pay for this again.)"""
        K = max(1, int(K))
        if (r, K) not in self._send_cache:
            self._send_cache[(r, K)] = self._send_schedule(r, K)
        return self._send_cache[(r, K)]

    def _send_schedule(self, r, K):
        n = self.i0[r].size
        b = self.chunk_bounds(n, K)
        sent = np.zeros(self.N, dtype=bool)
        sched = []
        for c in range(K):
            later = self._reach_of(self.i0[r][b[c + 1]:]) if c < K - 1 else np.zeros(self.N, dtype=bool)
            pieces = []
            for q in range(self.P):
                if q == r:
                    continue
                for a0, a1 in self.runs[r][q]:
                    ready = ~later[a0:a1] & ~sent[a0:a1]
                    for s0, s1 in _runs_of(ready):
                        pieces.append((q, a0 + s0, a0 + s1))
                        sent[a0 + s0:a0 + s1] = True
            sched.append(pieces)
        return sched

    def recv_schedule(self, q, K):
        """rsched[c] = [(r, a, b), ...]: what the other ranks send to q after their chunk c (rank order).  Memoised."""
        if (q, int(K)) not in self._recv_cache:
            self._recv_cache[(q, int(K))] = self._recv_schedule(q, K)
        return self._recv_cache[(q, int(K))]

    def _recv_schedule(self, q, K):
        out = [[] for _ in range(max(1, int(K)))]
        for r in range(self.P):
            if r == q:
                continue
            for c, pieces in enumerate(self.send_schedule(r, K)):
                out[c] += [(r, a, b) for (dest, a, b) in pieces if dest == q]
        return out

    def work_runs(self, r):
        """Planes rank r zeroes its accumulators on and forms nHI on: what its sources reach plus what it owns.  Memoised."""
        if r not in self._work_cache:
            mask = self.reach[r].copy()
            a, b = self.own[r]
            mask[a:b] = True
            self._work_cache[r] = _runs_of(mask)
        return self._work_cache[r]

    def back_runs(self, r):
        """(sends, recvs) of rank r in the second exchange, each [(peer, a, b), ...] in rank order: the runs travel back -- r, as
        the owner, sends the new xh_av of runs[q][r] to every q that traces through them, and expects runs[r][q] from its owner q.
        Memoised."""
        if r not in self._back_cache:
            self._back_cache[r] = ([(q, a, b) for q in range(self.P) if q != r for a, b in self.runs[q][r]],
                                   [(q, a, b) for q in range(self.P) if q != r for a, b in self.runs[r][q]])
        return self._back_cache[r]

    def reach_runs(self, r):
        return _runs_of(self.reach[r])

    @staticmethod
    def _fields(thermal, exchange):
        """Grids that travel per plane: the rate exchange of a thermal step carries the heating rates too, the xh_av exchange never."""
        if exchange not in ("rates", "xh_av"):
            raise ValueError(f"exchange: 'rates' or 'xh_av', not {exchange!r}")
        return 2 if (thermal and exchange == "rates") else 1

    def bytes_per_rank(self, r, thermal=False, exchange="rates"):
        """(sent, received) by rank r in ONE of the two exchanges of an iteration, in bytes: `exchange` = "rates" (to the owners)
        or "xh_av" (back).  Isothermal, both move the same planes; in a `thermal` step every plane of the rate direction travels
        twice, as photo-ionisation and as heating rates, and the xh_av direction is unchanged."""
        plane = 8 * self.N * self.N * self._fields(thermal, exchange)
        sent = sum((b - a) for q in range(self.P) if q != r for a, b in self.runs[r][q])
        recv = sum((b - a) for q in range(self.P) if q != r for a, b in self.runs[q][r])
        return sent * plane, recv * plane

    def largest_transfer(self, thermal=False, exchange="rates"):
        """Bytes of the largest rank-to-rank transfer of one exchange (what a single xGMI link carries in one direction);
        `thermal`, `exchange` as in ``bytes_per_rank``."""
        plane = 8 * self.N * self.N * self._fields(thermal, exchange)
        return plane * max([sum(b - a for a, b in self.runs[r][q]) for r in range(self.P) for q in range(self.P) if q != r] or [0])


class _DevicePointer:
    """Zero-copy view of a library-owned device buffer for torch (__cuda_array_interface__ v3)."""

    def __init__(self, ptr, nelem):
        self.__cuda_array_interface__ = {
            "shape": (int(nelem),), "typestr": "<f8", "data": (int(ptr), False), "version": 3, "strides": None,
        }


#: A grid that travels between ranks, as the NAMES of the library methods that reach it; `add`, `add_host` where planes that arrive
#: are ADDED instead of replacing what is there.  `args` go in front of the first three calls (the selector of a library grid).
_Field = collections.namedtuple("_Field", "ptr to_host from_host add add_host args", defaults=(None, None, ()))

#: the out-boxes of the device-resident loop; a thermal step sends both, per run of planes the rates first
_RATES = _Field("evolve_slab_outbox_ptr", "evolve_slab_outbox_to_host", "evolve_slab_outbox_from_host",
                "evolve_slab_add", "evolve_slab_add_host")
_HEAT = _Field("evolve_slab_heat_outbox_ptr", "evolve_slab_heat_outbox_to_host", "evolve_slab_heat_outbox_from_host",
               "evolve_slab_add_heat", "evolve_slab_add_heat_host")


def _grid(which):
    """The library grid `which`; planes that arrive replace what is there."""
    return _Field("device_ptr", "planes_to_host", "planes_to_device", args=(int(which),))


def _call(lib, name, *args):
    return getattr(lib, name)(*args)


class _Rccl:
    """RCCL ("nccl"): the library's buffers are zero-copy views and everything is ordered on the library's stream -- sends start
    behind the kernels that produced the planes, the stream waits for a transfer, never the host."""
    device = "cuda"

    def __init__(self, dist, group):
        import torch
        self._torch, self._dist, self._group = torch, dist, group
        self._views, self._sums, self._rounds = {}, {}, {}
        self._lib_stream = self._lib_stream_ptr = self._comm_stream = None

    def fence(self, libasora=None):
        """The host waits for the library's stream, or for the device."""
        if libasora is not None:
            libasora.synchronize()
        else:
            self._torch.cuda.synchronize()

    def phase_stream(self, libasora):
        """The library's stream; its events delimit the phases of an iteration."""
        ptr = libasora.stream_ptr()
        if self._lib_stream_ptr != ptr:
            self._lib_stream, self._lib_stream_ptr = self._torch.cuda.ExternalStream(ptr), ptr
        return self._lib_stream

    def stream(self, libasora):
        return self._torch.cuda.stream(self.phase_stream(libasora))

    def _view(self, libasora, field, N):
        """Zero-copy (N, N*N) view of a field; kept per (address, N): the grids do not move between iterations."""
        ptr = _call(libasora, field.ptr, *field.args)
        if (ptr, N) not in self._views:
            self._views[(ptr, N)] = self._torch.as_tensor(_DevicePointer(ptr, N ** 3), device="cuda").view(N, N * N)
        return self._views[(ptr, N)]

    def round(self, libasora, fields, N, key, build):
        """build() once per `key` and addresses of the fields: buffers, targets and P2POp list are the same every iteration."""
        key += tuple((f, self._view(libasora, f, N).data_ptr()) for f in fields)
        if key not in self._rounds:
            self._rounds[key] = build()
        return self._rounds[key]

    def outgoing(self, libasora, field, a, b, N):
        return self._view(libasora, field, N)[a:b]

    def incoming(self, libasora, field, a, b, N):
        if field.add:
            return self._torch.empty((b - a, N * N), dtype=self._torch.float64, device="cuda")
        return self._view(libasora, field, N)[a:b]

    def deliver(self, libasora, field, a, b, t):
        if field.add:
            _call(libasora, field.add, a, b - a, t.data_ptr())

    def all_reduce_field(self, libasora, field, N):
        self._dist.all_reduce(self._view(libasora, field, N), op=self._dist.ReduceOp.SUM, group=self._group)

    def broadcast_planes(self, libasora, field, a, b, N, src):
        self._dist.broadcast(self._view(libasora, field, N)[a:b], src=src, group=self._group)

    def sum_and_close(self, libasora):
        """The three sums of this rank's pass all-reduced in place where the library keeps them."""
        ptr = libasora.reduction_ptr()
        if ptr not in self._sums:
            self._sums[ptr] = self._torch.as_tensor(_DevicePointer(ptr, 3), device="cuda")
        with self.stream(libasora):
            self._dist.all_reduce(self._sums[ptr], op=self._dist.ReduceOp.SUM, group=self._group)
        libasora.evolve_slab_close(None)

    @contextlib.contextmanager
    def beside_trace(self, libasora, field, N):
        """Yields reduce(a, b, gate): the planes [a, b) summed on a second stream once the library's stream gets to the call, while
        the trace goes on; `gate`: the library's stream then waits for the sum.  On leaving it waits for every sum."""
        torch = self._torch
        lib_stream = self.phase_stream(libasora)
        if self._comm_stream is None:
            self._comm_stream = torch.cuda.Stream()
        comm_stream, view = self._comm_stream, self._view(libasora, field, N)

        def reduce(a, b, gate):
            done = torch.cuda.Event()
            done.record(lib_stream)                        # the planes are final once the library stream gets here
            comm_stream.wait_event(done)
            with torch.cuda.stream(comm_stream):
                self._dist.all_reduce(view[a:b], op=self._dist.ReduceOp.SUM, group=self._group)
            if gate:
                summed = torch.cuda.Event()
                summed.record(comm_stream)
                lib_stream.wait_event(summed)
        yield reduce
        lib_stream.wait_stream(comm_stream)                # whatever follows on the library stream needs the sums


class _Gloo:
    """gloo (CPU tests, several ranks on one GPU): everything is staged through the host, which waits for every transfer."""
    device = "cpu"

    def __init__(self, dist, group):
        import torch
        self._torch, self._dist, self._group = torch, dist, group
        self._me = dist.get_rank(group)

    def fence(self, libasora=None):
        pass

    def phase_stream(self, libasora):
        return None                                        # the phases are wall-clock spans between host synchronisations

    def stream(self, libasora):
        return contextlib.nullcontext()

    def round(self, libasora, fields, N, key, build):
        return build()                                     # what leaves is copied to the host anew every iteration

    def outgoing(self, libasora, field, a, b, N):
        return self._torch.from_numpy(_call(libasora, field.to_host, *field.args, a, b - a, N))

    def incoming(self, libasora, field, a, b, N):
        return self._torch.empty((b - a, N, N), dtype=self._torch.float64)

    def deliver(self, libasora, field, a, b, t):
        if field.add_host:
            _call(libasora, field.add_host, a, t.numpy())
        else:
            _call(libasora, field.from_host, *field.args, a, t.numpy())

    def all_reduce_field(self, libasora, field, N):
        self._round_trip_sum(libasora, field, N, 0, N)

    def _round_trip_sum(self, libasora, field, N, a, b):
        """The planes [a, b) summed over the ranks; the whole grid makes the round trip through the host."""
        # (a library grid has calls of its own for the whole of it)
        host = libasora.grid_to_host(*field.args, np.empty((N, N, N))) if field.args else _call(libasora, field.to_host, 0, N, N)
        self._dist.all_reduce(self._torch.from_numpy(host[a:b]), op=self._dist.ReduceOp.SUM, group=self._group)
        if field.args:
            libasora.grid_to_device(*field.args, host)
        else:
            _call(libasora, field.from_host, 0, host)

    def broadcast_planes(self, libasora, field, a, b, N, src):
        t = self.outgoing(libasora, field, a, b, N) if src == self._me else self.incoming(libasora, field, a, b, N)
        self._dist.broadcast(t, src=src, group=self._group)
        if src != self._me:
            self.deliver(libasora, field, a, b, t)

    def sum_and_close(self, libasora):
        part = libasora.chemistry_finish()                      # (conv_flag, sum x, sum 1-x) of this rank
        t = self._torch.tensor([float(part[0]), float(part[1]), float(part[2])], dtype=self._torch.float64)
        self._dist.all_reduce(t, op=self._dist.ReduceOp.SUM, group=self._group)
        v = t.tolist()
        libasora.evolve_slab_close((v[0], v[1], v[2]))

    @contextlib.contextmanager
    def beside_trace(self, libasora, field, N):
        yield lambda a, b, gate: self._round_trip_sum(libasora, field, N, a, b)


class _Phases:
    """Where one multi-rank iteration spends its time (``TorchComm.phase_timing``; bench.py's ``phases_ms``).

    With RCCL everything an iteration does is ordered on the library's stream, transfers included (the stream waits for
    them, not the host), so a phase is the span between two events recorded on that stream: time the GPU spent on it
    INCLUDING what it waited for -- `wait_rates_add` is the part of the rate exchange the trace did not hide.  The events
    are resolved later (``TorchComm.phase_report``), never inside an iteration.  With gloo (CPU rehearsals) the planes go
    through the host and every phase ends with a host synchronisation and a wall-clock reading."""

    def __init__(self, comm, libasora):
        self._comm, self._lib, self._clock = comm, libasora, time.perf_counter
        self._stream = comm._t.phase_stream(libasora)
        self._device = self._stream is not None
        if self._device:
            import torch
            self._torch = torch
            self._events = [("", self._record())]
        else:
            libasora.synchronize()
            self._t = self._clock()

    def _record(self):
        e = self._torch.cuda.Event(enable_timing=True)
        e.record(self._stream)
        return e

    def mark(self, name):
        """The phase `name` ends here."""
        if self._device:
            self._events.append((name, self._record()))
        else:
            self._lib.synchronize()
            t = self._clock()
            self._comm._phase_add(name, (t - self._t) * 1e3)
            self._t = t

    def close(self):
        self._comm._phase_n += 1
        if self._device:
            self._comm._phase_pending.append(self._events)
            if len(self._comm._phase_pending) >= 512:
                self._comm._phase_resolve()


class TorchComm:
    """Communicator over a torch.distributed process group; what RCCL and gloo do differently is in ``_Rccl`` / ``_Gloo``."""

    def __init__(self, group=None, overlap=None, chunks=8, pipeline_chemistry=None):
        import torch.distributed as dist
        if not dist.is_initialized():
            raise RuntimeError("TorchComm: torch.distributed is not initialised "
                               "(call pyc2ray_amd.dist.init_process_group_from_env() first)")
        self._dist = dist
        self._group = group
        self._t = (_Rccl if self._backend() == "nccl" else _Gloo)(dist, group)
        if overlap is None:
            overlap = os.environ.get("PYC2RAY_AMD_OVERLAP", "0") == "1"
        self.overlap = bool(overlap)
        self.chunks = int(os.environ.get("PYC2RAY_AMD_OVERLAP_CHUNKS", chunks))
        # also start each slab's chemistry behind its sum (measured on one GPU: the chemistry kernels then compete
        # with the trace for the memory system and the step gets 0.25 ms LONGER, so this stays off)
        if pipeline_chemistry is None:
            pipeline_chemistry = os.environ.get("PYC2RAY_AMD_OVERLAP_CHEMISTRY", "0") == "1"
        self.pipeline_chemistry = bool(pipeline_chemistry)
        #: how the per-rank rate grids are summed: "slab" (SlabPlan: planes to their owners, slab chemistry, xh_av
        #: back) or "allreduce" (full-grid all-reduce, chemistry replicated on every rank)
        self.exchange = os.environ.get("PYC2RAY_AMD_EXCHANGE", "slab")
        #: "allreduce" without `overlap`: True = on the device-resident loop (``reduce_begin``: batches of iterations per host round
        #: trip, as the slab exchange and the one-GPU loop); False = three calls and a host read-back per iteration
        self.device_loop = os.environ.get("PYC2RAY_AMD_REDUCE_LOOP", "1") != "0"
        #: slab exchange: trace chunks per iteration; planes that are final after a chunk travel while the next is traced
        # (measured per-rank compute + modelled links, tools/slab_compute_model.py, profiles/r03_slab_model_chunks.txt: splitting
        #  the trace costs more than the early sends hide from four ranks on -- 125 sources per launch no longer fill the chip
        #  -- and gains ~15 % with two ranks)
        self.slab_chunks = int(os.environ.get("PYC2RAY_AMD_SLAB_CHUNKS", "2" if self._dist.get_world_size(group) == 2 else "1"))
        #: every rank derives the convergence decision from the SAME all-reduced scalars (no broadcast of the decision needed)
        self.identical_scalars = True
        #: True: every iteration books where its time went (``_Phases``); read with ``phase_report``
        self.phase_timing = False
        self._phase_ms, self._phase_n, self._phase_pending = {}, 0, []
        # the step of the device-resident loop that is under way (``_begin``): (plan or None, N, local sources), the out-boxes that travel
        self._slab, self._rate_fields = None, (_RATES,)
        # Bring the communicator up with a collective EVERY rank takes part in.  The slab exchange is point-to-point
        # and a rank with nothing to send or receive skips it; if that were the first operation on the process group,
        # the ranks that do take part would wait for the others in the communicator's set-up.
        dist.all_reduce(self._tensor([0.0]), group=self._group)

    # -- mpi4py-flavoured surface ---------------------------------------------------------------
    def Get_rank(self):
        return self._dist.get_rank(self._group)

    def Get_size(self):
        return self._dist.get_world_size(self._group)

    def Barrier(self):
        self._dist.barrier(self._group)

    @staticmethod
    def _buf(spec):
        return spec[0] if isinstance(spec, (list, tuple)) else spec

    def _backend(self):
        return self._dist.get_backend(self._group)

    @property
    def backend(self):
        """"nccl" (RCCL: exchanges on the device, batches of iterations per host round trip) or "gloo" (through the host)."""
        return self._backend()

    def _tensor(self, values, dtype=None):
        """A few scalars where this backend's collectives take them; float64 unless told otherwise."""
        import torch
        return torch.tensor(values, dtype=dtype or torch.float64, device=self._t.device)

    def _tensor_of(self, arr):
        import torch
        return torch.from_numpy(np.ascontiguousarray(arr)).to(self._t.device)

    def Allreduce(self, sendbuf, recvbuf, op=None):
        """Sum-allreduce of a numpy buffer (mpi4py calling convention, IN_PLACE supported)."""
        out = self._buf(recvbuf)
        in_place = isinstance(sendbuf, str) and sendbuf == MPI.IN_PLACE
        src = out if in_place else self._buf(sendbuf)
        t = self._tensor_of(src)
        self._dist.all_reduce(t, op=self._dist.ReduceOp.SUM, group=self._group)
        out[...] = t.cpu().numpy().reshape(out.shape)

    def Reduce(self, sendbuf, recvbuf, op=None, root=0):
        """Sum-reduce to `root` (evolve.py:433-436 convention: root passes IN_PLACE + its buffer)."""
        in_place = isinstance(sendbuf, str) and sendbuf == MPI.IN_PLACE
        src = self._buf(recvbuf) if in_place else self._buf(sendbuf)
        t = self._tensor_of(src)
        self._dist.reduce(t, dst=root, op=self._dist.ReduceOp.SUM, group=self._group)
        if self.Get_rank() == root:
            out = self._buf(recvbuf)
            out[...] = t.cpu().numpy().reshape(out.shape)

    def Bcast(self, buf, root=0):
        arr = self._buf(buf)
        a = np.asarray(arr)
        t = self._tensor_of(a)
        self._dist.broadcast(t, src=root, group=self._group)
        res = t.cpu().numpy().reshape(a.shape)
        if isinstance(arr, np.ndarray):
            arr[...] = res
        else:                       # array.array and friends (evolve.py:484-487)
            for i, v in enumerate(res.ravel()):
                arr[i] = v.item()

    # -- the data-path collective -------------------------------------------------------------------
    def _collective(self):
        """Whether a sum over the ranks is carried out: always with more than one; PYC2RAY_AMD_FORCE_COLLECTIVE=1 lets a 1-GPU
        box exercise the collective path."""
        return self.Get_size() > 1 or os.environ.get("PYC2RAY_AMD_FORCE_COLLECTIVE", "0") == "1"

    def allreduce_device_grid(self, libasora, which, N):
        """In-place sum over ranks of the device-resident grid `which` (N^3 float64); the host waits for it."""
        if not self._collective():
            return
        self._t.fence(libasora)
        with self._t.stream(libasora):
            self._t.all_reduce_field(libasora, _grid(which), N)
        self._t.fence()

    # -- diagnostics: per-phase times of an iteration, measured link rates ----------------------------------------
    def _phase_add(self, name, ms):
        self._phase_ms[name] = self._phase_ms.get(name, 0.0) + ms

    def _phase_resolve(self):
        if not self._phase_pending:
            return
        import torch
        torch.cuda.synchronize()
        for events in self._phase_pending:
            for (_, e0), (name, e1) in zip(events[:-1], events[1:]):
                self._phase_add(name, e0.elapsed_time(e1))
        self._phase_pending = []

    def phase_reset(self):
        self._phase_resolve()
        self._phase_ms, self._phase_n = {}, 0

    def phase_report(self, reduce_max=True):
        """Mean milliseconds per iteration of every phase booked since ``phase_reset`` -- the MAXIMUM over the ranks when
        `reduce_max` (a collective: every rank must call it), plus "iterations".  Phase names: slab exchange --
        trace_fold_post, wait_rates_add, slab_pass, xh_av_exchange_nhi, scalar_allreduce_test; all-reduce loop -- trace_fold,
        rate_allreduce, pass_test; pipelined all-reduce (raytrace_and_allreduce) -- trace, rate_allreduce, chemistry."""
        self._phase_resolve()
        names = sorted(self._phase_ms)
        n = max(self._phase_n, 1)
        vals = [self._phase_ms[k] / n for k in names]
        if reduce_max and self.Get_size() > 1:
            # (ranks on different exchange paths would book different names: the caller keeps them on one path)
            t = self._tensor(vals)
            self._dist.all_reduce(t, op=self._dist.ReduceOp.MAX, group=self._group)
            vals = t.cpu().tolist()
        out = dict(zip(names, vals))
        out["iterations"] = self._phase_n
        return out

    def _ring(self, snd, rcv):
        """One round of the neighbour ring: every rank sends `snd` to its right neighbour and receives `rcv` from its left one,
        through ``batch_isend_irecv`` as the slab exchange does."""
        dist = self._dist
        P, me = self.Get_size(), self.Get_rank()
        ops = [dist.P2POp(dist.isend, snd, (me + 1) % P, group=self._group),
               dist.P2POp(dist.irecv, rcv, (me - 1) % P, group=self._group)]
        for w in dist.batch_isend_irecv(ops):
            w.wait()

    def measure_links(self, p2p_bytes=16 << 20, allreduce_bytes=128 << 20, reps=3, p2p=True):
        """What the links of THIS job deliver, through the calls the data path uses: a ring of point-to-point transfers of
        `p2p_bytes` (``_ring``) and an in-place sum all-reduce of `allreduce_bytes` (the full-grid exchange).  One untimed round
        each, then the fastest of `reps`; times are the MAXIMUM over the ranks, so every rank returns the same numbers and
        derives the same choice from them.  p2p = False leaves the ring out (a caller whose point-to-point preflight failed:
        the all-reduce time is still worth having).  Returns {"p2p_bytes", "p2p_ms", "p2p_GBs" (per link and direction),
        "allreduce_bytes", "allreduce_ms", "allreduce_busbw_GBs" (2 (P-1)/P bytes / time, the ring's per-link rate)}."""
        import torch
        dist, fence, dev = self._dist, self._t.fence, self._t.device
        P, me = self.Get_size(), self.Get_rank()

        def timed(fn):
            best = None
            for rep in range(reps + 1):
                dist.barrier(self._group)
                fence()
                t0 = time.perf_counter()
                fn()
                fence()
                dt = time.perf_counter() - t0
                if rep > 0:
                    best = dt if best is None else min(best, dt)
            t = self._tensor([best])
            dist.all_reduce(t, op=dist.ReduceOp.MAX, group=self._group)
            return float(t.item())

        out = {"p2p_bytes": int(p2p_bytes), "allreduce_bytes": int(allreduce_bytes), "ranks": P, "backend": self._backend()}
        if P < 2:
            out.update(p2p_ms=None, p2p_GBs=None, allreduce_ms=None, allreduce_busbw_GBs=None)
            return out
        n1 = max(1, int(p2p_bytes) // 8)
        snd = torch.full((n1,), float(me + 1), dtype=torch.float64, device=dev)
        rcv = torch.zeros((n1,), dtype=torch.float64, device=dev)
        t_p2p = timed(lambda: self._ring(snd, rcv)) if p2p else None
        n2 = max(1, int(allreduce_bytes) // 8)
        buf = torch.zeros((n2,), dtype=torch.float64, device=dev)
        t_ar = timed(lambda: dist.all_reduce(buf, op=dist.ReduceOp.SUM, group=self._group))
        del buf, snd, rcv
        out.update(p2p_ms=t_p2p * 1e3 if p2p else None, p2p_GBs=8.0 * n1 / t_p2p / 1e9 if p2p else None,
                   allreduce_ms=t_ar * 1e3, allreduce_busbw_GBs=2.0 * (P - 1) / P * 8.0 * n2 / t_ar / 1e9)
        return out

    def preflight_p2p(self, nelem=65536):
        """One small round of the neighbour ring (``_ring``) through the same call the slab exchange uses.  The exchange has
        never run between real GPUs on the build box; a caller that gets an exception here (or False from any rank, after a
        MIN-reduce of the results) takes the all-reduce path.  Returns True when the round went through on this rank and the
        payload arrived intact."""
        import torch
        P, me = self.Get_size(), self.Get_rank()
        if P < 2:
            return True
        out = torch.full((nelem,), float(me + 1), dtype=torch.float64, device=self._t.device)
        inc = torch.zeros((nelem,), dtype=torch.float64, device=self._t.device)
        self._ring(out, inc)
        self._t.fence()
        return bool((inc == float((me - 1) % P + 1)).all().item())

    # -- slab exchange: rates to the owners of the planes, ionised fraction back (see SlabPlan) -------------------
    @staticmethod
    def shard_sources_by_slab(src_pos, src_flux, nprocs, src_spectrum=None):
        """Order the source list by its first coordinate and cut it into the reference's contiguous blocks
        (pyc2ray/evolve.py:362-367: perrank = NumSrc // nprocs, the last rank takes the remainder).  Returns
        (src_pos, src_flux, bounds) with rank r holding [bounds[r], bounds[r+1]) of the reordered list; with `src_spectrum`
        (the spectrum of each source) a fourth element, reordered like the other two."""
        pos, flux = np.asarray(src_pos), np.asarray(src_flux)
        order = np.argsort(pos[0], kind="stable")
        n = flux.shape[0]
        per = n // nprocs
        bounds = [r * per for r in range(nprocs)] + [n]
        spectra = () if src_spectrum is None else (np.asarray(src_spectrum)[order],)
        return (pos[:, order], flux[order], bounds) + spectra

    def _post(self, libasora, fields, N, sends, recvs, tag):
        """Start one round of plane transfers: `sends` = [(peer, a, b)] planes [a, b) to peer, `recvs` likewise from peer; per
        run every field travels, in the order of `fields`.  Returns a handle for ``_complete``; `tag` tells an iteration's rounds apart."""
        if not sends and not recvs:
            return None
        dist, t = self._dist, self._t

        def build():
            out = [[t.outgoing(libasora, f, a, b, N) for f in fields] for _, a, b in sends]
            targets = [[t.incoming(libasora, f, a, b, N) for f in fields] for _, a, b in recvs]
            ops = [dist.P2POp(dist.isend, x, q, group=self._group) for (q, _, _), xs in zip(sends, out) for x in xs]
            ops += [dist.P2POp(dist.irecv, x, q, group=self._group) for (q, _, _), xs in zip(recvs, targets) for x in xs]
            return targets, ops
        with t.stream(libasora):
            targets, ops = t.round(libasora, fields, N, (tag, N, tuple(sends), tuple(recvs)), build)
            works = dist.batch_isend_irecv(ops)
        return works, ops, fields, recvs, targets

    def _complete(self, libasora, handle):
        """Wait for a round started by ``_post`` and deliver what arrived: in the order of `recvs` (rank order), per run in the
        order of the fields -- a fixed order of additions, the same bits on every run."""
        if handle is None:
            return
        works, _, fields, recvs, targets = handle
        with self._t.stream(libasora):
            for w in works:
                w.wait()
        for (_, a, b), ts in zip(recvs, targets):
            for f, x in zip(fields, ts):
                self._t.deliver(libasora, f, a, b, x)

    # -- the device-resident loop over several ranks (asora_evolve_slab_*, include/asora_hip.h) ------------------------
    def _begin(self, libasora, plan, own, N, R, sig, dr, num_src_local, minlogtau, dlogtau, NumTau, chemistry, conv_criterion,
               convergence_fraction, thermal):
        """A time step of the device-resident loop on the planes own = [a, b) of this rank."""
        a, b = own
        begin = libasora.evolve_begin_slab_thermal if thermal else libasora.evolve_begin_slab
        begin(*chemistry, R, sig, dr, minlogtau, dlogtau, NumTau, 0, num_src_local, conv_criterion, convergence_fraction, a, b - a)
        self._slab = (plan, int(N), int(num_src_local))
        self._rate_fields = (_RATES, _HEAT) if thermal else (_RATES,)

    def slab_begin(self, libasora, plan, N, R, sig, dr, num_src_local, minlogtau, dlogtau, NumTau, chemistry,
                   conv_criterion, convergence_fraction, thermal=False):
        """Start a time step of the sharded loop: NDENS, TEMP, XH and this rank's sources are on the device.  `chemistry` =
        (dt, bh00, albpow, colh0, temph0, abu_c); conv_criterion from the TOTAL source count (pyc2ray/evolve.py:127,346).
        thermal = True: the library is in thermal mode (``ThermalParams.apply``), the step is begun through
        asora_evolve_begin_slab_thermal and the first exchange carries the heating planes with the rate planes."""
        self._begin(libasora, plan, plan.own[self.Get_rank()], N, R, sig, dr, num_src_local, minlogtau, dlogtau, NumTau, chemistry,
                    conv_criterion, convergence_fraction, thermal)

    def reduce_begin(self, libasora, N, R, sig, dr, num_src_local, minlogtau, dlogtau, NumTau, chemistry, conv_criterion,
                     convergence_fraction, thermal=False):
        """Start a time step of the same device-resident loop with the reference's exchange (pyc2ray/evolve.py:433-437): every
        rank traces its sources, the rate grid is all-reduced, every rank runs the chemistry of the WHOLE grid on identical
        rates (and so takes the same decisions without exchanging anything else).  ``slab_enqueue`` / ``slab_poll`` drive it.
        thermal = True (the library in thermal mode): both out-boxes, rates and heating, are all-reduced."""
        self._begin(libasora, None, (0, N), N, R, sig, dr, num_src_local, minlogtau, dlogtau, NumTau, chemistry, conv_criterion,
                    convergence_fraction, thermal)

    def thermal_stats(self, libasora):
        """asora_thermal_stats of the thermal step just run, for the whole grid and the same on every rank: (cells that hit
        max_substeps, cells clamped to t_floor, most substeps of one integration).  Slab exchange: every rank has integrated its
        own planes, so the two counts are summed over the ranks and the third is their maximum (a collective: every rank calls
        it).  All-reduce loop: every rank has computed the whole grid on identical rates, its own numbers are the answer."""
        import torch
        capped, floored, most = libasora.thermal_stats()
        if self._slab[0] is None or self.Get_size() == 1:
            return capped, floored, most
        counts, top = self._tensor([capped, floored], torch.int64), self._tensor([most], torch.int64)
        self._dist.all_reduce(counts, op=self._dist.ReduceOp.SUM, group=self._group)
        self._dist.all_reduce(top, op=self._dist.ReduceOp.MAX, group=self._group)
        c = counts.cpu().tolist()
        return int(c[0]), int(c[1]), int(top.cpu().item())

    def _reduce_one(self, libasora):
        """One iteration of the loop begun with ``reduce_begin``: trace -> both accumulator layouts of all planes folded into
        the out-box -> the out-box (a thermal step: then the heating out-box) summed over the ranks in place -> the fused pass
        on the whole grid reading the out-box (it keeps the summed rates in PHI_ION) -> convergence test on the pass's own
        sums.  With RCCL the all-reduce is ordered on the library's stream and nothing waits on the host; with gloo the out-box
        goes through the host."""
        _, N, num_src_local = self._slab
        ph = _Phases(self, libasora) if self.phase_timing else None
        libasora.evolve_slab_trace(0, num_src_local)
        libasora.evolve_slab_fold_all()
        if ph: ph.mark("trace_fold")
        if self._collective():
            with self._t.stream(libasora):
                for f in self._rate_fields:
                    self._t.all_reduce_field(libasora, f, N)
        if ph: ph.mark("rate_allreduce")
        libasora.evolve_slab_pass()
        libasora.evolve_slab_close(None)             # (the pass's sums are those of the whole grid, the same on every rank)
        if ph:
            ph.mark("pass_test")
            ph.close()

    def slab_enqueue(self, libasora, iterations=1):
        """Enqueue outer iterations of the step begun with ``slab_begin``.  One iteration = what the one-GPU loop does -- the
        trace and ONE fused pass -- with two plane exchanges in between:

          trace (in K chunks; after each, the foreign planes no later chunk reaches are folded into the out-box and sent to
          their owners) -> received rates added on the own planes -> fused pass on the own planes (rates folded, chemistry,
          nHI in both layouts, next accumulators zeroed) -> new xh_av of the planes other ranks trace through sent back, nHI
          formed on the halo planes as they arrive -> the three convergence sums all-reduced IN PLACE on the device and the
          test of evolve.py:216-236 evaluated there.

        With RCCL nothing here waits on the host: transfers, kernels and the test are ordered on the library's stream, every
        launch is gated by the device's `done` flag, and every rank evaluates the test on identical bits, so all ranks stop
        at the same iteration; ``slab_poll`` reads the status back once per batch.  With gloo (CPU rehearsals) the planes
        and the sums are staged through the host, one synchronisation per exchange."""
        one = self._reduce_one if self._slab[0] is None else self._slab_one
        for _ in range(int(iterations)):
            one(libasora)

    def slab_poll(self, libasora, max_rows=32):
        """(iterations carried out, converged, rows) -- asora_evolve_poll; folds the last iteration's rates into PHI_ION
        (complete on the own planes; ``slab_gather`` collects the owners' slabs at the end of the step)."""
        return libasora.evolve_poll(max_rows)

    def _slab_one(self, libasora):
        plan, N, num_src_local = self._slab
        me = self.Get_rank()
        # every rank walks through the same number of rounds and derives every other rank's schedule: the chunk count is a
        # function of the plan, never of this rank alone
        K = plan.common_chunks(self.slab_chunks)
        ph = _Phases(self, libasora) if self.phase_timing else None
        sched, rsched = plan.send_schedule(me, K), plan.recv_schedule(me, K)
        bounds = plan.chunk_bounds(num_src_local, K)
        handles = []
        for c in range(K):
            libasora.evolve_slab_trace(bounds[c], bounds[c + 1] - bounds[c])
            for _, a, b in sched[c]:
                libasora.evolve_slab_fold_out(a, b - a)                 # the planes that leave now
            # out-box planes to their owners, foreign contributions to the own planes into receive buffers
            handles.append(self._post(libasora, self._rate_fields, N, sched[c], rsched[c], c))
        if ph: ph.mark("trace_fold_post")
        for h in handles:                                               # chunk order, then rank order: a fixed order of additions
            self._complete(libasora, h)
        if ph: ph.mark("wait_rates_add")
        libasora.evolve_slab_pass()
        if ph: ph.mark("slab_pass")
        # xh_av back: the owner q of a run sends it to the rank r that traces through it; nHI there once it has arrived
        sends, recvs = plan.back_runs(me)
        self._complete(libasora, self._post(libasora, (_grid(_capi.GRID_XH_AV),), N, sends, recvs, "xh_av"))
        for _, a, b in recvs:
            libasora.evolve_slab_nhi(a, b - a)
        if ph: ph.mark("xh_av_exchange_nhi")
        self._t.sum_and_close(libasora)       # the three sums of this rank's pass summed over the ranks, then the test on the device
        if ph:
            ph.mark("scalar_allreduce_test")
            ph.close()

    def slab_iteration(self, libasora, plan, N, R, sig, dr, num_src_local, minlogtau, dlogtau, NumTau, chemistry, first):
        """ONE outer iteration and its three sums (conv_flag, sum x, sum 1-x) over the WHOLE grid, identical on every rank:
        ``slab_begin`` (when `first`; with a convergence test that never passes) + ``slab_enqueue(1)`` + ``slab_poll``.  For
        callers that drive the loop themselves; evolve3D_MPI and bench.py enqueue batches instead."""
        if first:
            self.slab_begin(libasora, plan, N, R, sig, dr, num_src_local, minlogtau, dlogtau, NumTau, chemistry, -1.0, 0.0)
        self.slab_enqueue(libasora, 1)
        _, _, rows = self.slab_poll(libasora, 1)
        return int(rows[-1][0]), float(rows[-1][1]), float(rows[-1][2])

    def slab_gather(self, libasora, plan, which, N):
        """Every rank gets every owner's slab of grid `which` (end of a time step: xh_intermed, phi_ion; a thermal step:
        temp_end and phi_heat as well)."""
        with self._t.stream(libasora):
            for q, (a, b) in enumerate(plan.own):
                if b > a:
                    self._t.broadcast_planes(libasora, _grid(which), a, b, N, q)

    # -- raytrace + sum over ranks, optionally pipelined ------------------------------------------------
    @staticmethod
    def sort_sources_for_overlap(src_pos, src_flux, src_spectrum=None):
        """Order a rank's sources by their first coordinate (what the pipelined path needs).  src_pos is
        (3, n) 1-based; returns (src_pos, src_flux) reordered -- and `src_spectrum`, the spectrum of each source, when
        given.  The sum over sources is order-independent up to floating-point rounding."""
        order = np.argsort(np.asarray(src_pos)[0], kind="stable")
        spectra = () if src_spectrum is None else (np.asarray(src_spectrum)[order],)
        return (np.asarray(src_pos)[:, order], np.asarray(src_flux)[order]) + spectra

    @staticmethod
    def final_plane_runs(N, chunks, R, c, reduced):
        """Planes of the rate grid that are final once the sources of chunks 0..c (sources with 0-based first
        coordinate < (c+1)*N//chunks) have been traced and that have not been summed yet, as a list of
        half-open runs.  A later source sits at i >= (c+1)*N//chunks and reaches the planes i-R..i+R, wrapping
        at most onto planes < R; the last chunk releases everything that is left.  Depends on (N, chunks, R)
        only, so every rank derives the same runs."""
        margin = int(np.ceil(R)) + 1
        if c == chunks - 1:
            want = ~reduced
        else:
            want = np.zeros(N, dtype=bool)
            lo, hi = margin, (c + 1) * N // chunks - margin
            if hi > lo:
                want[lo:hi] = True
            want &= ~reduced
        return _runs_of(want)

    def raytrace_and_allreduce(self, libasora, N, R, sig, dr, num_src_local, minlogtau, dlogtau, NumTau,
                               src_i0=None, chemistry=None):
        """Trace this rank's sources and leave the sum over ranks of the rate grids in the device-resident
        phi_ion grid.  Pipelined when self.overlap is set and `src_i0` (0-based first coordinates of the local
        sources, ascending, in upload order) is given; otherwise trace, then all-reduce.

        With `chemistry` = (dt, bh00, albpow, colh0, temph0, abu_c) the chemistry pass is run as well and its
        (conv_flag, sum x, sum 1-x) returned; with self.pipeline_chemistry each slab's chemistry starts as soon as its
        rates are summed, under the remaining trace and all-reduces."""
        if not self.overlap or src_i0 is None:
            # three calls; with `phase_timing`, between wall-clock readings (all but the trace end with a host synchronisation anyway)
            stamps = []

            def mark(sync=False):
                if self.phase_timing:
                    if sync: libasora.synchronize()
                    stamps.append(time.perf_counter())
            mark()
            libasora.raytrace_device(R, sig, dr, 0, num_src_local, minlogtau, dlogtau, NumTau)
            mark(sync=True)
            self.allreduce_device_grid(libasora, _capi.GRID_PHI_ION, N)
            mark()
            res = libasora.chemistry_device(*chemistry) if chemistry is not None else None
            mark()
            for name, t0, t1 in zip(("trace", "rate_allreduce", "chemistry"), stamps, stamps[1:]):
                self._phase_add(name, (t1 - t0) * 1e3)
            self._phase_n += bool(stamps)
            return res
        src_i0 = np.asarray(src_i0)
        if src_i0.size and np.any(np.diff(src_i0) < 0):
            raise ValueError("raytrace_and_allreduce: sources must be uploaded in ascending order of their first "
                             "coordinate (TorchComm.sort_sources_for_overlap)")
        K = max(1, min(self.chunks, N))
        starts = np.searchsorted(src_i0, [c * N // K for c in range(K + 1)], side="left")
        starts[-1] = src_i0.size
        reduced = np.zeros(N, dtype=bool)
        first_slab = True
        slab_chemistry = chemistry is not None and self.pipeline_chemistry
        # reduce(a, b, gate): the planes [a, b), final now, summed over the ranks beside the rest of the trace
        sums = self._t.beside_trace(libasora, _grid(_capi.GRID_PHI_ION), N) if self._collective() else contextlib.nullcontext()
        with sums as reduce:
            libasora.raytrace_begin(R, sig, dr, minlogtau, dlogtau, NumTau)
            for c in range(K):
                libasora.raytrace_range(int(starts[c]), int(starts[c + 1] - starts[c]))
                for a, b in self.final_plane_runs(N, K, R, c, reduced):
                    libasora.raytrace_fold(a, b - a)
                    reduced[a:b] = True
                    if reduce is not None:
                        reduce(a, b, slab_chemistry)           # the slab's chemistry goes behind its sum
                    if slab_chemistry:
                        libasora.chemistry_range(*chemistry, a, b - a, first_slab)
                        first_slab = False
            assert reduced.all()
        if chemistry is None:
            return None
        return libasora.chemistry_finish() if slab_chemistry else libasora.chemistry_device(*chemistry)
