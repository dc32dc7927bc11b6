"""Drop-in for the reference's voxel_processor.py: same class, same methods, same argument meaning
(/root/reference/voxel_processor.py:27-164), computed by the HIP kernels of libtomo_hip.so.

Host arrays in, host arrays out (the reference's consumers need real np.ndarray); the bit-packed
device copy of every returned volume is cached (see _devcache: returned volumes are write-protected, a
writeable array is verified byte for byte before its cached copy is used) so the orchestrator's next call does
not upload it again.  There is no CPU fallback: without a GPU / the built library these methods raise.
"""
import os
import sys
import threading

import numpy as np
import torch

from . import _devcache, _hostbuf, _memo, pipeline


def _device():
    if not torch.cuda.is_available():
        raise pipeline._lib.TomoUnavailable("no MI355X visible: the HIP path has no CPU fallback")
    return torch.device("cuda", torch.cuda.current_device())


def to_device_volume(voxel_data):
    """ndarray (nz,ny,nx) -> BitVolume, via the cache when the array came from this package."""
    vol = _devcache.get(voxel_data) if isinstance(voxel_data, np.ndarray) else None
    if vol is not None:
        return vol
    return upload_volume(voxel_data)


def with_device_volume(voxel_data, fn):
    """fn(vol) with the device copy of `voxel_data`.  A remembered copy of a WRITEABLE array (the default kind of result) is
    used speculatively: its byte-for-byte verification (a checksum of the whole array, 5-6 ms per GiB) runs on a helper thread
    NEXT TO fn -- the device work and the download of fn's result -- and fn runs again on a fresh upload if the array turns out
    to have been edited.  fn must have no effect but its return value."""
    if isinstance(voxel_data, np.ndarray):
        vol, check = _devcache.get_deferred(voxel_data)
        if vol is not None:
            res = fn(vol)
            if check is None or check():
                return res
    return fn(upload_volume(voxel_data))


def upload_volume(voxel_data):
    """ndarray (nz,ny,nx) -> a FRESH BitVolume (never the cached one: the caller may overwrite it)."""
    a = np.ascontiguousarray(voxel_data)
    if a.ndim != 3:
        raise ValueError("voxel data must be 3-D")
    if a.dtype != np.bool_:
        a = a != 0
    t = torch.from_numpy(a.view(np.uint8)).to(_device(), non_blocking=True)
    return pipeline.pack(t)


_NP_OF = {torch.bool: np.bool_, torch.uint8: np.uint8, torch.float32: np.float32, torch.float64: np.float64, torch.int64: np.int64,
          torch.int32: np.int32}


BIG = 1 << 28        # bytes from which a transfer goes straight from / into ordinary (pageable) memory: ROCm page-locks a large
#                      pageable buffer on the fly (1 GiB: 21 ms against 19 ms page-locked), smaller ones pass through its staging
#                      buffers at a fraction of the bus rate -- those use torch's page-locked cache (a few ms to lock, once)


def to_host_array(t):
    """Device tensor -> fresh host ndarray.  Volume-sized results are ordinary NumPy arrays whose pages many threads have
    brought in (_hostbuf: page-locking a fresh gibibyte costs ~65 ms, the first run of a process would pay it three times);
    mesh-sized ones are NumPy views of page-locked torch tensors."""
    if t.numel() * t.element_size() >= BIG:
        out = _hostbuf.take(tuple(t.shape), _NP_OF[t.dtype])
        torch.from_numpy(out).copy_(t)          # ordered after the current stream's work; returns when the bytes are there
        return out
    host = torch.empty(t.shape, dtype=t.dtype, pin_memory=True)
    host.copy_(t, non_blocking=True)
    torch.cuda.current_stream().synchronize()
    return host.numpy()


PIECE = 128 << 20   # bytes per piece of a download that is checksummed on the way (a whole number of checksum chunks)
_DIGEST_POOL = []


def _download_with_digest(t):
    """to_host_array for a volume-sized tensor whose checksum is wanted as well (writeable results: _devcache verifies them
    at the next lookup): the download runs in pieces of PIECE bytes and piece k is digested by a helper thread (native, threaded;
    the foreign call releases the interpreter lock) while piece k + 1 is on the bus -- the 5-6 ms a checksum of 1 GiB costs
    disappear behind the 20 ms of its download.  -> (host ndarray, digest as _devcache.checksum gives it)."""
    import ctypes
    from concurrent.futures import ThreadPoolExecutor
    L = pipeline._lib.lib()
    out = _hostbuf.take(tuple(t.shape), _NP_OF[t.dtype])
    flat_h = out.reshape(-1).view(np.uint8)
    flat_d = t.reshape(-1).view(torch.uint8)
    n = flat_h.shape[0]
    chunk = int(L.tomo_host_checksum_chunk_bytes())
    piece = max(chunk, PIECE // chunk * chunk)
    nchunks = -(-n // chunk)
    dig = np.zeros(2 * nchunks + 2, dtype=np.uint64)
    nt = max(1, min(16, os.cpu_count() or 1))
    if not _DIGEST_POOL:
        _DIGEST_POOL.append(ThreadPoolExecutor(1, thread_name_prefix="tomo-digest"))

    def digest(a, b):
        pipeline._lib.check(L.tomo_host_checksum_part(flat_h[a:b].ctypes.data, b - a, a // chunk, nt, 0,
                                                      dig[2 * (a // chunk):].ctypes.data), "tomo_host_checksum_part")
    futs = []
    for a in range(0, n, piece):
        b = min(n, a + piece)
        torch.from_numpy(flat_h[a:b]).copy_(flat_d[a:b])      # ordered after the current stream's work; returns when the bytes are there
        futs.append(_DIGEST_POOL[0].submit(digest, a, b))
    for f in futs:
        f.result()
    res = (ctypes.c_uint64 * 2)()
    pipeline._lib.check(L.tomo_host_checksum_fold(dig.ctypes.data, nchunks, n, res), "tomo_host_checksum_fold")
    return out, (int(res[0]), int(res[1]))


def to_host_volume(vol):
    """BitVolume -> fresh host bool ndarray, remembered against its device copy (writeable and checksummed by default;
    write-protected under TOMO_READONLY_RESULTS)."""
    t = pipeline.unpack(vol)
    if _devcache.WRITEABLE_RESULTS and t.numel() * t.element_size() >= BIG:
        out, digest = _download_with_digest(t)
        _devcache.put(out, vol, digest=digest)
        return out
    out = to_host_array(t)
    _devcache.put(out, vol)
    return out


_STAGE = {}          # the staging array of the last upload, kept for the next one of the same size: a fresh gibibyte costs its
#                      page faults on the way in AND ~25 ms of munmap on the way out (measured: tools/h2hprof.py)
_STAGE_LOCK = threading.Lock()
_STAGE_TIMER = [None]
STAGE_IDLE_S = 20.0  # ... but not for ever: an idle staging array goes back to the system after this long (a timer, not the
#                      next call: a process that made its one create_voxel_data must not sit on a volume-sized array)
STAGE_KEEP_MAX = int(os.environ.get("TOMO_STAGE_KEEP_MAX", str(8 << 30)))   # larger staging arrays are never kept between calls


def _release_staging():
    with _STAGE_LOCK:
        _STAGE.clear()
        _STAGE_TIMER[0] = None


def _staging(shape):
    key = (threading.get_ident(), tuple(shape))
    with _STAGE_LOCK:
        a = _STAGE.get(key)
        if a is None:
            _STAGE.clear()                      # one staging array per process: another shape replaces it
            a = np.empty(shape, dtype=np.bool_)
            if a.nbytes <= STAGE_KEEP_MAX:
                _STAGE[key] = a
        if _STAGE_TIMER[0] is not None:
            _STAGE_TIMER[0].cancel()
        if _STAGE:
            t = _STAGE_TIMER[0] = threading.Timer(STAGE_IDLE_S, _release_staging)
            t.daemon = True
            t.start()
    return a


def _stage_masks(mask_images):
    """np.stack(mask_images) (voxel_processor.py:46) straight into a page-locked staging tensor, copied by a few host
    threads (NumPy releases the GIL while copying) and uploaded chunk by chunk behind them: (nz, ny, nx) uint8 0/1 on
    the device."""
    from concurrent.futures import ThreadPoolExecutor
    first = np.asarray(mask_images[0])
    if first.ndim != 2:
        raise ValueError("all input arrays must have the same shape")          # what np.stack reports for ragged input
    nz = len(mask_images)
    # np.stack into ONE staging array (ordinary memory: its pages are brought in by the copying workers themselves, in
    # parallel), cut into chunks of slices; every chunk is uploaded as soon as its host copy is done, so the PCIe transfer
    # runs under the host copies of the later chunks.  (Rounds 1-2 staged through page-locked memory: 68 ms of page-locking
    # in front of the first call of a process, for a transfer that is as fast from pageable memory on this platform.)
    stage = _staging((nz,) + first.shape)
    # uploads in pieces of >= 128 MiB (below that ROCm stages a pageable source through its own buffers at a fraction of the
    # bus rate; above it the source is page-locked on the fly: 1 GiB in 8 pieces 19 ms, in 32 pieces 90-120 ms)
    per_slice = int(first.size)             # bytes per mask (bool); create_voxel_data keeps zero-size stacks away from here
    if per_slice == 0:
        raise ValueError("zero-size masks have nothing to stage")
    up = max(1, min(nz, -(-(128 << 20) // per_slice)))                                           # slices per upload piece
    dev = torch.empty((nz,) + first.shape, dtype=torch.bool, device=_device())
    # Fast path (what an image loader produces: separate C-contiguous bool / uint8-of-0/1... arrays of one shape): the
    # stacking is a native multi-threaded gather (tomo_host_gather) -- piece k + 1 is gathered on a helper thread while
    # piece k is on the bus.  (Python worker threads copying slice by slice took 17-60 ms for the same gibibyte, at the
    # mercy of the interpreter lock; np.stack itself 85 ms.)
    L = pipeline._lib.lib()
    ptrs = np.empty(nz, dtype=np.uintp)
    plain = True
    for i, m in enumerate(mask_images):
        if not (isinstance(m, np.ndarray) and m.dtype == np.bool_ and m.shape == first.shape and m.flags.c_contiguous):
            plain = False
            break
        ptrs[i] = m.__array_interface__["data"][0]
    nthreads = max(1, min(16, os.cpu_count() or 1))
    if plain:
        def gather(lo, hi):
            pipeline._lib.check(L.tomo_host_gather(ptrs[lo:hi].ctypes.data, hi - lo, per_slice, stage[lo:hi].ctypes.data, nthreads),
                                "tomo_host_gather")
        with ThreadPoolExecutor(1) as ex:          # measured (tools/h2hprof.py): gather 1.2-1.5 ms, upload 2.4-2.9 ms per 128 MiB
            spans = [(lo, min(nz, lo + up)) for lo in range(0, nz, up)]
            futs = [ex.submit(gather, lo, hi) for lo, hi in spans]
            for (lo, hi), fut in zip(spans, futs):
                fut.result()
                dev[lo:hi].copy_(torch.from_numpy(stage[lo:hi]))
        return dev.view(torch.uint8)
    workers = max(1, min(8, os.cpu_count() or 1, nz))
    fine = max(1, -(-up // workers))                                                           # slices per worker task

    def fill(lo, hi):
        for i in range(lo, hi):
            m = np.asarray(mask_images[i])
            if m.shape != first.shape:
                raise ValueError("all input arrays must have the same shape")
            stage[i] = m if m.dtype == np.bool_ else (m != 0)
    with ThreadPoolExecutor(workers) as ex:
        pieces = []
        for lo in range(0, nz, up):
            hi = min(nz, lo + up)
            pieces.append((lo, hi, [ex.submit(fill, a, min(hi, a + fine)) for a in range(lo, hi, fine)]))
        for lo, hi, futs in pieces:
            for fut in futs:
                fut.result()
            dev[lo:hi].copy_(torch.from_numpy(stage[lo:hi]))
    return dev.view(torch.uint8)


def _common_base(mask_images):
    """If the masks are the consecutive slices (views) of ONE contiguous (nz, ny, nx) array -- what this package's
    ImageLoader hands out -- return that array: np.stack would only copy it."""
    first = mask_images[0]
    base = getattr(first, "base", None)
    if not (isinstance(first, np.ndarray) and isinstance(base, np.ndarray) and base.ndim == 3 and
            base.shape[0] == len(mask_images) and base.flags.c_contiguous and base.dtype == first.dtype):
        return None
    ptr0, step = base.__array_interface__["data"][0], base.strides[0]
    for i, m in enumerate(mask_images):
        if not (isinstance(m, np.ndarray) and m.base is base and m.shape == base.shape[1:] and
                m.strides == base.strides[1:] and m.__array_interface__["data"][0] == ptr0 + i * step):
            return None
    return base


POINT_CLOUD_WINDOW_BYTES = 1 << 30      # device memory one download window of generate_point_cloud holds at most


def _point_cloud_host(voxel_data, mm_per_pixel_x, mm_per_pixel_y, slice_depths, subsample_factor=1):
    """voxel_processor.py:99-127 in NumPy."""
    z, y, x = np.where(voxel_data)
    if subsample_factor > 1:
        idx = np.arange(0, len(z), subsample_factor)
        z, y, x = z[idx], y[idx], x[idx]
    d = np.asarray(slice_depths, dtype=np.float64)
    cum = np.cumsum(np.concatenate([[0], d]))
    if len(d):
        zc = np.minimum(z, len(d) - 1)
        z_mm = np.where(z < len(d), cum[zc] + d[zc] / 2, cum[-1])
    else:
        z_mm = np.full(len(z), cum[-1])
    return np.column_stack([z_mm, y * mm_per_pixel_y, x * mm_per_pixel_x])


def _plain_scale(v, extent):
    """A scale the kernel's `(double)index * (double)scale` reproduces for indices below `extent`: NumPy multiplies the int64
    indices by a float scale in float64, and by an int scale in int64 -- the same value while the product stays below 2^53."""
    if isinstance(v, (float, np.float64, np.float32)):
        return True
    return isinstance(v, (int, np.integer)) and abs(int(v)) * extent < 2 ** 53


def _point_cloud_on_device(voxel_data, mm_per_pixel_x, mm_per_pixel_y, subsample_factor):
    if not (isinstance(voxel_data, np.ndarray) and voxel_data.ndim == 3 and voxel_data.dtype == np.bool_ and voxel_data.size > 0):
        return False
    nz, ny, nx = voxel_data.shape
    return (isinstance(subsample_factor, (int, np.integer)) and _plain_scale(mm_per_pixel_x, nx) and _plain_scale(mm_per_pixel_y, ny)
            and nz * ny * ((nx + 63) // 64) < 2 ** 31                       # the kernels index words with 32 bits (TOMO_E_SIZE beyond)
            and torch.cuda.is_available() and os.path.exists(pipeline._lib.SO_PATH))


def _point_cloud_device(voxel_data, mm_per_pixel_x, mm_per_pixel_y, slice_depths, subsample_factor):
    vol = to_device_volume(voxel_data)
    plan = pipeline.PointCloudPlan(vol, pipeline.point_cloud_z_table(slice_depths, vol.shape[0]), mm_per_pixel_y, mm_per_pixel_x,
                                   pipeline.point_cloud_step(subsample_factor))
    rows = plan.n_rows
    step = max(1, POINT_CLOUD_WINDOW_BYTES // 24)
    if rows == 0:
        return np.empty((0, 3), dtype=np.float64)
    if rows <= step:
        return to_host_array(plan.rows())
    out = _hostbuf.take((rows, 3), np.float64)
    for a in range(0, rows, step):
        b = min(rows, a + step)
        torch.from_numpy(out[a:b]).copy_(plan.rows(a, b))        # returns when the bytes are there: one window resident at a time
    return out


def _env_count(name):
    """A non-negative integer from the environment (unset / empty: 0); anything else is an error, not a silent default."""
    text = os.environ.get(name, "").strip()
    if not text:
        return 0
    value = int(text)
    if value < 0:
        raise ValueError("%s must be a non-negative integer" % name)
    return value


class VoxelProcessor:
    """Handles voxel data creation and processing operations (reference: voxel_processor.py:27).

    Optional, beyond the reference: island removal.  Three instance attributes (TOMO_MIN_COMPONENT_VOXELS=N and
    TOMO_KEEP_LARGEST=1 in the environment set the first two for every new object, which is how the unchanged orchestrator
    gets them): with min_component_voxels > 0 or keep_largest_component set, every volume create_voxel_data and
    smooth_voxel_data hand out holds only the connected components (component_connectivity 6 or 26, scipy.ndimage.label's
    meaning) of at least that many voxels, respectively only the largest of those.  Off by default: nothing is launched then.

    Likewise optional: filling enclosed cavities.  fill_cavities (TOMO_FILL_CAVITIES=1) and max_cavity_voxels
    (TOMO_MAX_CAVITY_VOXELS=N; 0: no limit): every volume handed out has its enclosed voids -- those of at most that many voxels
    -- filled (pipeline.fill_cavities under component_connectivity), after the islands are gone and, in smooth_voxel_data,
    after the smoothing, because a closing can seal a void.  Off by default: nothing is launched then."""

    def __init__(self):
        self.voxel_data = None
        self.side_0_count = 0
        self.side_1_count = 0
        self.side_2_count = 0
        self.min_component_voxels = _env_count("TOMO_MIN_COMPONENT_VOXELS")
        self.keep_largest_component = os.environ.get("TOMO_KEEP_LARGEST", "0") not in ("", "0")
        self.component_connectivity = 6
        self.fill_cavities = os.environ.get("TOMO_FILL_CAVITIES", "0") not in ("", "0")
        self.max_cavity_voxels = _env_count("TOMO_MAX_CAVITY_VOXELS")

    def _component_options(self):
        """(min voxels, largest, connectivity) when island removal is on, else None."""
        n, largest = int(self.min_component_voxels), bool(self.keep_largest_component)
        if n <= 0 and not largest:
            return None
        if self.component_connectivity not in pipeline.CONNECTIVITIES:
            raise ValueError("component_connectivity must be 6 or 26")
        return max(n, 0), largest, int(self.component_connectivity)

    def _fill_options(self):
        """(connectivity, largest cavity filled or None) when cavity filling is on, else None."""
        if not self.fill_cavities:
            return None
        n = int(self.max_cavity_voxels)
        if n < 0:
            raise ValueError("max_cavity_voxels must be a non-negative integer")
        if self.component_connectivity not in pipeline.CONNECTIVITIES:
            raise ValueError("component_connectivity must be 6 or 26")
        return int(self.component_connectivity), n if n > 0 else None

    def _keep_components(self, vol):
        """`vol` without its islands, then with its cavities filled (a new volume), or `vol` itself when both options are off."""
        opts, fill = self._component_options(), self._fill_options()
        if opts is not None:
            vol = pipeline.keep_components(vol, *opts)
        if fill is not None:
            vol = pipeline.fill_cavities(vol, fill[0], 0, fill[1])
        return vol

    def create_voxel_data(self, mask_images: list, close_ends: bool = True,
                          side_0_count: int = 0, side_1_count: int = 0, side_2_count: int = 0) -> np.ndarray:
        """voxel_processor.py:36-54."""
        if not mask_images:
            raise ValueError("Load masks first, hmm.")
        self.side_0_count = side_0_count
        self.side_1_count = side_1_count
        self.side_2_count = side_2_count
        if np.asarray(mask_images[0]).size == 0:
            # masks without a single pixel (shape (0, k) / (k, 0)): nothing to upload, close or count -- np.stack as the reference
            # does (voxel_processor.py:46; a ragged list raises its ValueError), closing the ends of an empty volume changes nothing
            self.voxel_data = np.stack(mask_images, axis=0)
            print(f"Voxels: {self.voxel_data.shape}, active: {int(np.sum(self.voxel_data)):,}")
            return self.voxel_data
        base = _common_base(mask_images)
        cached = _devcache.get(base) if base is not None else None
        if close_ends and torch.cuda.is_available():
            # the 1 B/voxel host arrays this call and the smooth_voxel_data that follows it hand back: their pages are brought in
            # NOW, on helper threads, next to the upload
            _hostbuf.reserve(len(mask_images) * np.asarray(mask_images[0]).size, count=2)
        if cached is not None and not base.flags.writeable and any(m.flags.writeable for m in mask_images):
            # writeable views of a protected stack: its content may have changed behind the flag -- the remembered device
            # copy is dropped for good (a later lookup must not find it either) and the stack is uploaded again
            _devcache.invalidate(base)
            cached = None
        if close_ends:
            if cached is not None:                           # uploaded (and thresholded) by ImageLoader already: closed into a COPY
                vol = pipeline.close_ends(cached)
            elif base is not None:
                vol = pipeline.close_ends(upload_volume(base), inplace=True)           # a fresh upload, never a cached volume: ours to overwrite
            else:
                vol = pipeline.pack_closed(_stage_masks(mask_images))
            vol = self._keep_components(vol)                 # after the ends are closed; the count below is the filtered one
            active = int(pipeline.popcount_async(vol).item())
            self.voxel_data = to_host_volume(vol)
        else:
            stacked = np.stack(mask_images, axis=0)          # the reference returns a new array here
            vol = cached if cached is not None else upload_volume(stacked)
            if self._component_options() is not None or self._fill_options() is not None:
                vol = self._keep_components(vol)             # the array handed out is the download of the filtered volume
                active = int(pipeline.popcount_async(vol).item())
                self.voxel_data = to_host_volume(vol)
            else:
                active = int(pipeline.popcount_async(vol).item())
                self.voxel_data = stacked
                _devcache.put(stacked, vol)
        print(f"Voxels: {self.voxel_data.shape}, active: {active:,}")
        return self.voxel_data

    def smooth_voxel_data(self, voxel_data: np.ndarray, iterations: int = 3, create_manifold: bool = True) -> np.ndarray:
        """voxel_processor.py:79-97 (binary_opening + `iterations` x binary_closing, 3-D cross).  Like the reference
        (:93-95) a failure of the full sequence falls back to the closings alone; only a missing GPU / library raises
        on the first attempt (there is no CPU path to fall back to)."""
        def work(vol):
            try:
                # the orchestrator repeats this very call several times: the device result is remembered (see _memo), the
                # host array is a fresh download every time
                key = (int(iterations), bool(create_manifold), opts)
                sm = _memo.smoothed.get(vol, key)
                if sm is None:
                    sm = self._keep_components(pipeline.smooth(vol, iterations, create_manifold))   # opening can detach a piece
                    _memo.smoothed.put(vol, key, sm)
                return to_host_volume(sm)
            except pipeline._lib.TomoUnavailable:
                raise
            except Exception as e:                                       # noqa: BLE001 -- the reference catches Exception here
                print(f"tomography_3d_reconstructor_amd: smoothing failed ({e}); closings only", file=sys.stderr)
                return to_host_volume(self._keep_components(pipeline.smooth(vol, iterations, False)))
        opts = (self._component_options(), self._fill_options())
        return with_device_volume(voxel_data, work)

    def generate_point_cloud(self, voxel_data: np.ndarray, mm_per_pixel_x: float, mm_per_pixel_y: float,
                             slice_depths: np.ndarray, subsample_factor: int = 1) -> np.ndarray:
        """voxel_processor.py:99-127 (the orchestrator's fallback when there is no surface -- on the largest stacks).  A 3-D
        bool array with a GPU in sight is ranked and selected on the device, from the bit-packed copy (the cached one if this
        package handed the array out), and the float64 rows come down in windows of POINT_CLOUD_WINDOW_BYTES at most; anything
        else -- no GPU, another dtype, a non-integer factor, 2^31 words or more, no device memory -- is the reference's NumPy,
        unchanged.  Any other failure of the device path (a failed launch, a TomoError) raises: it is never hidden behind NumPy."""
        if _point_cloud_on_device(voxel_data, mm_per_pixel_x, mm_per_pixel_y, subsample_factor):
            try:
                return _point_cloud_device(voxel_data, mm_per_pixel_x, mm_per_pixel_y, slice_depths, subsample_factor)
            except torch.cuda.OutOfMemoryError:
                pass
        return _point_cloud_host(voxel_data, mm_per_pixel_x, mm_per_pixel_y, slice_depths, subsample_factor)

    def calculate_slice_depths(self, total_depth_mm: float) -> np.ndarray:
        """voxel_processor.py:129-164."""
        s0, s1, s2 = self.side_0_count, self.side_1_count, self.side_2_count
        total = s0 + s1 + s2
        if s1 == 0 or total == 0:
            if total == 0:
                return np.array([])
            return np.full(total, total_depth_mm / total)
        d1 = total_depth_mm / s1
        d02 = 2 * d1
        d0 = d02 / s0 if s0 > 0 else 0
        d2 = d02 / s2 if s2 > 0 else 0
        depths = [d0] * s0 + [d1] * s1 + [d2] * s2
        print(f"Slice depth sequence: Side_0[0-{s0-1}], Side_1[{s0}-{s0+s1-1}], Side_2[{s0+s1}-{len(depths)-1}]")
        return np.array(depths)
