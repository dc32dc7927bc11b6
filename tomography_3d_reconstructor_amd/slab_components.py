"""Connected components of a stack that is cut along z into slabs, one per rank: scipy.ndimage.label's numbering and sizes of
the WHOLE stack on every rank, the labels and the kept volume slab by slab, without gathering a slice wider than bits.

The rule: rank r labels its slab with pipeline.ComponentRuns (n_r components) and local
component c gets the global id base_r + c, base_r = n_0 + .. + n_(r-1).  Ids then ascend in the raster order of the pieces'
first voxels, pieces that touch across a cut are united larger-root-under-smaller, and numbering the roots in ascending id is
SciPy's numbering.  Three collective steps, every message size known to both ends from the step before:

  1  all-gather of 4 int64: n_r, the runs of the first and of the last slice, the guard flags of the local labelling
  2  exchange upward: the last slice as bits + one int32 per run of it (the run's local component); the receiver unites
     the ids of the runs that touch across the cut in a WINDOW of the id table (only ids of ranks r - 1 and r can meet there)
  3  all-gather of [seam flags | the sizes of the local components | the window]; every rank folds the windows into one
     table, numbers the roots, sums the sizes (tomo_cc_merge_tables) and holds the same n and sizes

Guard flags travel inside steps 1 and 3, so every rank raises the same TomoError at the same point and none is left waiting."""
import torch

from . import _lib, pipeline
from .pipeline import COUNTERS, BitVolume, _download, _p, _stream

F_HOST = 8       # flag bit next to the kernels' CC_F_* bits: the local labelling raised on the host (too many runs)


class SlabComponents:
    """Collective: every rank constructs it with its own slab (a BitVolume) and the same connectivity; `comm` only has to
    know the rank order (rank, world, exchange, all_gather).  n / sizes() are those of the whole stack, labels() / keep()
    this rank's slices.  events: a list that receives (name, torch.cuda.Event) marks at the phase boundaries (tools)."""

    def __init__(self, vol: BitVolume, comm, connectivity=6, events=None):
        if connectivity not in pipeline.CONNECTIVITIES:
            raise ValueError("connectivity must be 6 or 26")
        if not torch.cuda.is_available() or vol.bits is None or not vol.bits.is_cuda:
            raise _lib.TomoUnavailable("no MI355X visible: the HIP path has no CPU fallback")
        self.vol, self.comm, self.connectivity, self.events = vol, comm, int(connectivity), events
        self.rank, self.world = int(comm.rank), int(comm.world)
        self.bytes_published = 0
        self.n = 0
        nz, ny, nx = vol.shape
        dev = vol.device
        L = _lib.lib()
        self._mark("start")

        # ---- local labelling + step 1
        head = torch.zeros(4, dtype=torch.int64, device=dev)
        try:
            self.runs = pipeline.ComponentRuns(vol, self.connectivity)
        except _lib.TomoError:
            self.runs = None
            head[3] = F_HOST
        r = self.runs
        if r is not None and r.runs:
            ro = r.row_off
            head[0], head[3] = r.tot[1], r.tot[2]
            head[1] = ro[ny]
            head[2] = ro[nz * ny] - ro[(nz - 1) * ny]
        self._mark("local")
        heads = torch.stack([h.reshape(-1) for h in self._all_gather(head)]).cpu().tolist()      # the host read of step 1
        ns, kfirst, klast = ([int(h[k]) for h in heads] for k in range(3))
        flags = 0
        for h in heads:
            flags |= int(h[3])
        if flags or any(x < 0 for x in ns + kfirst + klast):
            raise _lib.TomoError("slab components: the local labelling of a rank failed (flags %d)" % flags)
        self.ns, self.bases = ns, [sum(ns[:k]) for k in range(self.world + 1)]
        self.n_total, self.n_local, self.base = self.bases[-1], ns[self.rank], self.bases[self.rank]
        if self.n_total >= pipeline.RUN_LIMIT:
            raise _lib.TomoError("slab components: too many components for 32-bit ids")
        COUNTERS["slab_components_label"] += 1
        if self.n_total == 0:                                # an empty stack: every rank knows, nobody sends anything
            self._mark("seam")
            return

        # ---- step 2: the last slice goes up, the seam below this slab is united
        me, nw = self.rank, ny * int(L.tomo_words_per_row(nx))
        n_prev = ns[me - 1] if me > 0 else 0
        wlen = n_prev + self.n_local if me > 0 else 0
        win, seam_tot = None, None
        if self.world > 1:
            up = torch.empty(nw + max(1, (klast[me] + 1) // 2), dtype=torch.int64, device=dev)
            up[:nw] = r.bits[nz - 1].reshape(-1)
            tail = up[nw:].view(torch.int32)
            if r.runs:
                _lib.check(L.tomo_cc_slice_components(nz, ny, nz - 1, *r._tables(), _p(r.tot), _p(tail), tail.numel(), _stream()),
                           "tomo_cc_slice_components")
            else:
                tail.zero_()
            shape = (nw + max(1, (klast[me - 1] + 1) // 2),) if me > 0 else None
            if me + 1 < self.world:
                self.bytes_published += up.numel() * 8
            below, _ = comm.exchange(None, up, torch.int64, recv_shape_prev=shape)
            if me > 0 and klast[me - 1] and kfirst[me]:
                if tuple(below.shape) != shape or below.dtype != torch.int64:
                    raise _lib.TomoError("slab components: rank %d received a seam message of the wrong size" % me)
                below = below.contiguous()
                nb_off = torch.empty(ny + 1, dtype=torch.int32, device=dev)
                blk = torch.empty(L.tomo_cc_scan_blocks(ny + 1), dtype=torch.int64, device=dev)
                nb_tot = torch.empty(8, dtype=torch.int64, device=dev)
                _lib.check(L.tomo_cc_count_runs(_p(below), 1, ny, nx, _p(nb_off), _p(blk), _p(nb_tot), _stream()), "tomo_cc_count_runs")
                win = torch.empty(wlen, dtype=torch.int32, device=dev)
                seam_tot = torch.empty(8, dtype=torch.int64, device=dev)
                _lib.check(L.tomo_cc_seam_union(_p(r.bits), ny, nx, self.connectivity, *r._tables(), _p(r.tot), _p(below), _p(nb_off),
                                                below[nw:].data_ptr(), klast[me - 1], n_prev, self.n_local, _p(win), _p(seam_tot),
                                                _stream()), "tomo_cc_seam_union")
                COUNTERS["slab_components_seam"] += 1
        self._mark("seam")

        # ---- step 3: seam flags, local sizes and the window to everybody; one table on every rank
        max_n = max(ns)
        max_win = max([ns[k - 1] + ns[k] for k in range(1, self.world)] or [0])
        off_win = 1 + max_n
        stride = off_win + (max_win + 1) // 2
        msg = torch.zeros(stride, dtype=torch.int64, device=dev)
        if self.n_local:
            msg[1:1 + self.n_local] = r._sizes[:self.n_local]
        if wlen:
            w32 = msg[off_win:].view(torch.int32)
            if win is None:
                w32[:wlen] = torch.arange(wlen, dtype=torch.int32, device=dev)
            else:
                w32[:wlen] = win
                msg[0] = seam_tot[2]
        rows = torch.stack([g.reshape(-1) for g in self._all_gather(msg)]).contiguous()
        if tuple(rows.shape) != (self.world, stride):
            raise _lib.TomoError("slab components: the gathered tables have the wrong size")
        N = self.n_total
        self.bases_dev = torch.tensor(self.bases, dtype=torch.int64, device=dev)
        self.table = torch.empty(N, dtype=torch.int32, device=dev)
        self.num = torch.empty(N, dtype=torch.int32, device=dev)
        self._sizes = torch.empty(N, dtype=torch.int64, device=dev)
        self.tot = torch.empty(8, dtype=torch.int64, device=dev)
        blk = torch.empty(L.tomo_cc_scan_blocks(N), dtype=torch.int64, device=dev)
        _lib.check(L.tomo_cc_merge_tables(_p(rows), self.world, stride, off_win, _p(self.bases_dev), N, max_n, max_win, _p(self.table),
                                          _p(self.num), _p(self._sizes), _p(blk), _p(self.tot), _stream()), "tomo_cc_merge_tables")
        host = _download(self.tot)                           # the same numbers on every rank: all raise, or none
        if host[2] or host[0] != N or not 0 < host[1] <= N:
            raise _lib.TomoError("slab components: the seam tables do not fit the slabs (flags %d)" % host[2])
        self.n = host[1]
        COUNTERS["slab_components_merge"] += 1
        self._mark("merge")

    def _mark(self, name):
        if self.events is not None:
            e = torch.cuda.Event(enable_timing=True)
            e.record(torch.cuda.current_stream())
            self.events.append((name, e))

    def _all_gather(self, t):
        self.bytes_published += t.numel() * t.element_size()
        return self.comm.all_gather(t)

    def _checked(self):
        """Raises when a guard fired in the work enqueued so far on this rank's tables or on the merged ones."""
        host = _download(torch.cat([self.runs.tot, self.tot]))
        if host[2] or host[0] != self.runs.runs or host[10]:
            raise _lib.TomoError("slab components: the run tables do not fit the volume (flags %d, %d)" % (host[2], host[10]))

    def _map(self, keep=None, label=None, min_voxels=0, largest=False):
        _lib.check(_lib.lib().tomo_cc_local_maps(_p(self.table), _p(self.num), _p(self._sizes), _p(self.tot), self.n_total, self.base,
                                                 self.n_local, min_voxels, int(bool(largest)), _p(keep), _p(label), _stream()),
                   "tomo_cc_local_maps")

    def sizes(self) -> torch.Tensor:
        """Voxels of component 1..n of the whole stack -> int64 (n,) device tensor, the same on every rank."""
        if self.n_total == 0:
            return torch.zeros(0, dtype=torch.int64, device=self.vol.device)
        return self._sizes[:self.n]

    def labels(self):
        """-> (int32 (nzl, ny, nx) device tensor: this rank's slices of scipy.ndimage.label's array of the whole stack, n)."""
        nz, ny, nx = self.vol.shape
        dev = self.vol.device
        COUNTERS["slab_components_expand"] += 1
        if self.n_local == 0:
            return torch.zeros((nz, ny, nx), dtype=torch.int32, device=dev), self.n
        r = self.runs
        label = torch.empty(self.n_local, dtype=torch.int32, device=dev)
        self._map(label=label)
        out = torch.empty((nz, ny, nx), dtype=torch.int32, device=dev)
        _lib.check(_lib.lib().tomo_cc_expand_map(_p(r.bits), nz, ny, nx, *r._tables(), _p(r.tot), _p(label), self.n_local, _p(out),
                                                 _stream()), "tomo_cc_expand_map")
        self._checked()
        return out, self.n

    def keep(self, min_voxels=0, largest=False) -> BitVolume:
        """A NEW volume of this rank's slices with the components of the WHOLE stack that have at least min_voxels voxels;
        largest: only the largest of those, the lowest global label among equals.  No collective step: any rank may call it."""
        nz, ny, nx = self.vol.shape
        dev = self.vol.device
        min_voxels = max(0, int(min_voxels))
        COUNTERS["slab_components_filter"] += 1
        self._mark("filter_start")
        if self.n_local == 0:
            return BitVolume(torch.zeros((nz, ny, int(_lib.lib().tomo_words_per_row(nx))), dtype=torch.int64, device=dev), self.vol.shape)
        r = self.runs
        keep = torch.empty(self.n_local, dtype=torch.uint8, device=dev)
        self._map(keep=keep, min_voxels=min_voxels, largest=largest)
        out = torch.empty_like(r.bits)
        _lib.check(_lib.lib().tomo_cc_filter_map(_p(r.bits), nz, ny, nx, *r._tables(), _p(r.tot), _p(keep), self.n_local, _p(out),
                                                 _stream()), "tomo_cc_filter_map")
        self._mark("filter")
        self._checked()
        return BitVolume(out, self.vol.shape)
