"""Fenced, poisoned device buffers for the tests: where do the kernels write, and what do they read before anyone wrote it?

    with fenced("ff", modules=(pipeline, slab)) as fz:
        with fz.unchanged(mask):
            vol = pipeline.pack_closed(mask)
        fz.check()

For its duration the global name `torch` of every listed module is a thin proxy.  It forwards everything to the real torch
except the allocating factories the package calls (FACTORIES below).  A device allocation made through one of them becomes

    | left fence, FENCE bytes | payload, nbytes | gap to the next multiple of ALIGN | right fence, FENCE bytes |

inside ONE uint8 base tensor from the real allocator.  Both fences and the gap hold PATTERN; the gap counts as right fence.
The payload comes back as a contiguous view of the requested shape and dtype (storage_offset != 0, data_ptr() % ALIGN == 0:
the alignment the caching allocator gives, which the kernels' wide accesses lean on).  The payload of `empty` / `empty_like`
is poisoned through its bytes -- "ff": 0xFF (floats are NaN, integers -1, bools 255), "rand": bytes of a generator seeded
with `seed`, the same for every allocation whatever thread made it, "zero": zeros (the control: it tells "a fence was
breached" from "garbage was read").  The payload of every other factory keeps its value and still gets fences.
check() synchronises, compares every fence with PATTERN on the device (one flag, one download), raises FenceBreach listing
every breached allocation (call site, shape, dtype, side, first and last modified fence offset) and drops the records.
Size-zero requests, CPU tensors (unless force_cpu=True: the harness's own tests) and pin_memory=True pass through untouched.

It is a module-level replacement, not a TorchDispatchMode: the slab tests run ranks as threads and dispatch modes are
thread-local.  A child process or a thread that cannot hold the `with` calls install() / uninstall() by hand.

NOT covered -- do not assume otherwise:
  * memory allocated inside tensor methods and operators (.clone(), .to(), .contiguous(), torch.cat / stack, indexing copies);
  * the hipMallocs inside libtomo_hip.so and the libraries it calls;
  * a breach further than FENCE bytes (4 KiB) from the buffer, and a write that happens to store PATTERN;
  * modules that are not listed, and names bound with `from torch import ...`.
"""
import os
import sys
import threading

import numpy as np
import torch as _torch

FENCE = 4096
ALIGN = 512
PATTERN = 0xA5
POISONS = ("ff", "rand", "zero")
EMPTY_FACTORIES = ("empty", "empty_like")
VALUE_FACTORIES = ("zeros", "zeros_like", "full", "full_like", "ones", "ones_like", "arange", "tensor")
FACTORIES = EMPTY_FACTORIES + VALUE_FACTORIES
_RAND_POOL = 1 << 16          # bytes of the "rand" poison; longer payloads repeat it
_HERE = os.path.abspath(__file__)


class FenceBreach(AssertionError):
    """check() found modified fence bytes; .breaches lists (record, side, first offset, last offset)."""

    def __init__(self, msg, breaches):
        super().__init__(msg)
        self.breaches = breaches


class Record:
    __slots__ = ("site", "shape", "dtype", "base", "off", "nbytes", "factory")

    def __init__(self, site, shape, dtype, base, off, nbytes, factory):
        self.site, self.shape, self.dtype, self.base, self.off, self.nbytes, self.factory = site, shape, dtype, base, off, nbytes, factory

    def left(self):
        return self.base[self.off - FENCE:self.off]

    def right(self):
        """The rounding gap behind the payload and the right fence: everything up to the end of the base."""
        end = self.off + self.nbytes
        return self.base[end:self.off + _round_up(self.nbytes) + FENCE]

    def describe(self):
        return "%s %s(%s, %s) %d bytes" % (self.site, self.factory, tuple(self.shape), str(self.dtype).replace("torch.", ""), self.nbytes)


def _round_up(n):
    return (n + ALIGN - 1) // ALIGN * ALIGN


def _call_site():
    f = sys._getframe(1)
    while f is not None and os.path.abspath(f.f_code.co_filename) == _HERE:
        f = f.f_back
    return "?" if f is None else "%s:%d in %s" % (os.path.basename(f.f_code.co_filename), f.f_lineno, f.f_code.co_name)


def _size_of(args):
    if len(args) == 1 and not isinstance(args[0], int):
        args = args[0]
    return tuple(int(s) for s in args)


class _Unchanged:
    """Snapshot of tensors; verify() (or leaving the `with`) asserts every one is byte-identical to its snapshot."""

    def __init__(self, tensors):
        self._pairs = [(t, t.detach().clone()) for t in tensors]

    def verify(self):
        for i, (t, snap) in enumerate(self._pairs):
            if t.device.type == "cuda":
                _torch.cuda.synchronize(t.device)
            same = t.shape == snap.shape and _torch.equal(t.contiguous().view(-1).view(_torch.uint8), snap.contiguous().view(-1).view(_torch.uint8))
            assert same, "input tensor %d %s %s was modified" % (i, tuple(t.shape), t.dtype)

    def __enter__(self):
        return self

    def __exit__(self, et, ev, tb):
        if et is None:
            self.verify()
        return False


class _Proxy:
    """Stands for the module `torch` inside the package: the factories of the harness, everything else the real thing."""

    def __init__(self, harness):
        self.__dict__["_harness"] = harness
        for name in FACTORIES:
            self.__dict__[name] = harness._factory(name)

    def __getattr__(self, name):
        return getattr(_torch, name)

    def __repr__(self):
        return "<fenced proxy of %r>" % (_torch,)


class Fenced:
    def __init__(self, poison="ff", modules=(), seed=0, force_cpu=False):
        if poison not in POISONS:
            raise ValueError("poison must be one of %s" % (POISONS,))
        self.poison, self.modules, self.seed, self.force_cpu = poison, tuple(modules), int(seed), bool(force_cpu)
        self.records = []
        self.total = 0                     # allocations fenced since install(), check() does not reset it
        self.sites = {}                    # call site -> allocations fenced there
        self._lock = threading.Lock()
        self._saved = None
        self._pools = {}
        self._rand = np.random.default_rng(self.seed).integers(0, 256, _RAND_POOL, dtype=np.uint8)
        self.proxy = _Proxy(self)

    # ------------------------------------------------------------------ installation
    def install(self):
        if self._saved is not None:
            raise RuntimeError("already installed")
        saved = []
        try:
            for m in self.modules:
                old = m.__dict__.get("torch")
                if old is not _torch:
                    raise RuntimeError("%s does not hold the real torch under the name `torch`" % m.__name__)
                saved.append((m, old))
                m.torch = self.proxy
        except BaseException:
            for m, old in saved:
                m.torch = old
            raise
        self._saved = saved
        return self

    def uninstall(self):
        saved, self._saved = self._saved, None
        for m, old in saved or ():
            m.torch = old

    def __enter__(self):
        return self.install()

    def __exit__(self, et, ev, tb):
        self.uninstall()
        self.records = []                  # without check(): the bases go back to the allocator
        return False

    # ------------------------------------------------------------------ allocation
    def _wanted(self, device, pin_memory=False):
        if pin_memory:
            return False
        return _torch.device(device).type == "cuda" or self.force_cpu

    def _pool(self, device):
        key = str(device)
        with self._lock:
            p = self._pools.get(key)
        if p is None:
            p = _torch.from_numpy(self._rand).to(device)
            with self._lock:
                p = self._pools.setdefault(key, p)
        return p

    def allocate(self, shape, dtype, device, factory, site, poison=True):
        """One fenced allocation -> the payload view.  shape with a zero: the caller passes through instead."""
        device = _torch.device(device)
        numel = 1
        for s in shape:
            numel *= s
        itemsize = _torch.empty(0, dtype=dtype).element_size()
        nbytes = numel * itemsize
        body = _round_up(nbytes)
        slack = 0 if device.type == "cuda" else ALIGN          # the host allocator aligns to 64 bytes only
        base = _torch.empty(FENCE + body + FENCE + slack, dtype=_torch.uint8, device=device)
        lead = -(base.data_ptr() + FENCE) % ALIGN
        if lead > slack:
            raise RuntimeError("the allocator returned a block that is not %d-byte aligned" % ALIGN)
        base = base[lead:lead + FENCE + body + FENCE]
        off = FENCE
        base[:off].fill_(PATTERN)
        base[off + nbytes:].fill_(PATTERN)
        raw = base[off:off + nbytes]
        if poison:
            if self.poison == "ff":
                raw.fill_(0xFF)
            elif self.poison == "zero":
                raw.zero_()
            else:
                pool = self._pool(device)
                for a in range(0, nbytes, _RAND_POOL):
                    n = min(_RAND_POOL, nbytes - a)
                    raw[a:a + n].copy_(pool[:n])
        out = raw.view(dtype).view(shape)
        assert out.is_contiguous() and out.storage_offset() != 0 and out.data_ptr() % ALIGN == 0
        rec = Record(site, tuple(shape), dtype, base, off, nbytes, factory)
        with self._lock:
            self.records.append(rec)
            self.total += 1
            self.sites[site] = self.sites.get(site, 0) + 1
        return out

    def _factory(self, name):
        real = getattr(_torch, name)
        like = name.endswith("_like")

        def empty(*args, **kw):
            extra = set(kw) - {"dtype", "device", "pin_memory"}
            if extra:
                raise NotImplementedError("fenced torch.%s: unsupported arguments %s" % (name, sorted(extra)))
            if like:
                (src,) = args
                shape, dtype, device = tuple(src.shape), kw.get("dtype") or src.dtype, kw.get("device") or src.device
            else:
                shape = _size_of(args)
                dtype = kw.get("dtype") or _torch.get_default_dtype()
                device = kw.get("device")
                device = _torch.device("cpu") if device is None else device
            if 0 in shape or not self._wanted(device, kw.get("pin_memory", False)):
                return real(*args, **kw)
            return self.allocate(shape, dtype, device, name, _call_site())

        def value(*args, **kw):
            r = real(*args, **kw)
            if r.numel() == 0 or r.layout != _torch.strided or r.is_pinned() or not self._wanted(r.device, kw.get("pin_memory", False)):
                return r
            out = self.allocate(tuple(r.shape), r.dtype, r.device, name, _call_site(), poison=False)
            out.copy_(r)
            return out

        fn = empty if name in EMPTY_FACTORIES else value
        fn.__name__ = fn.__qualname__ = name
        return fn

    # ------------------------------------------------------------------ checks
    def ran(self, function):
        """Allocations made inside the function of that name since install(): the proof that a path was taken."""
        with self._lock:
            return sum(n for site, n in self.sites.items() if site.endswith(" in " + function))

    def unchanged(self, *tensors):
        return _Unchanged(tensors)

    def check(self):
        """Every fence of every recorded allocation still holds PATTERN, else FenceBreach.  The records are dropped."""
        with self._lock:
            records, self.records = self.records, []
        devices = {}
        for r in records:
            devices.setdefault(r.base.device, []).append(r)
        dirty = False
        for device, recs in devices.items():
            if device.type == "cuda":
                _torch.cuda.synchronize(device)
            flag = _torch.zeros(1, dtype=_torch.int64, device=device)
            for r in recs:
                flag += (r.left() != PATTERN).sum() + (r.right() != PATTERN).sum()
            dirty = bool(int(flag.item())) or dirty
        if not dirty:
            return len(records)
        breaches = []
        for r in records:
            for side, fence in (("left", r.left()), ("right", r.right())):
                bad = np.flatnonzero(fence.cpu().numpy() != PATTERN)
                if len(bad):
                    # left: bytes BEFORE the payload's first byte (1 = the byte next to it); right: bytes past its last byte
                    first, last = (FENCE - int(bad[-1]), FENCE - int(bad[0])) if side == "left" else (int(bad[0]) + 1, int(bad[-1]) + 1)
                    breaches.append((r, side, first, last))
        lines = ["%d fence(s) breached under poison %r:" % (len(breaches), self.poison)]
        for r, side, first, last in breaches:
            lines.append("  %s: %s fence modified %d .. %d bytes %s the payload" % (r.describe(), side, first, last,
                                                                                   "before" if side == "left" else "past"))
        raise FenceBreach("\n".join(lines), breaches)


def fenced(poison="ff", modules=(), seed=0, force_cpu=False):
    """The context manager: `with fenced("ff", modules=(pipeline, slab)) as fz`."""
    return Fenced(poison, modules, seed, force_cpu)


def package_modules():
    """The modules of the package that allocate device memory through the name `torch`."""
    from tomography_3d_reconstructor_amd import glb_exporter, image_loader, pipeline, rccl, slab, surface_extractor, voxel_processor
    return (pipeline, slab, voxel_processor, surface_extractor, glb_exporter, image_loader, rccl)
