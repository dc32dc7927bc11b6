"""tests/fenced.py, the allocation harness of test_gpu_fenced.py, tested without a GPU: force_cpu=True sends CPU allocations
through the code the device allocations take."""
import os
import sys
import threading
import types

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fenced as F  # noqa: E402

DTYPES = [torch.uint8, torch.bool, torch.int16, torch.int32, torch.int64, torch.float32, torch.float64]
SHAPES = [(1,), (7,), (3, 5), (2, 3, 65), (513,), (4096,)]


def _module():
    m = types.ModuleType("fenced_probe")
    m.torch = torch
    return m


@pytest.fixture
def mod():
    return _module()


def _ok(t, shape, dtype):
    assert tuple(t.shape) == tuple(shape) and t.dtype == dtype
    assert t.is_contiguous() and t.data_ptr() % F.ALIGN == 0 and t.storage_offset() != 0
    assert t.device.type == "cpu"


@pytest.mark.parametrize("dtype", DTYPES)
def test_returned_tensors(mod, dtype):
    with F.fenced("zero", (mod,), force_cpu=True) as fz:
        for shape in SHAPES:
            _ok(mod.torch.empty(shape, dtype=dtype), shape, dtype)
            _ok(mod.torch.empty(*shape, dtype=dtype, device="cpu"), shape, dtype)
            src = torch.ones(shape, dtype=dtype)
            _ok(mod.torch.empty_like(src), shape, dtype)
            z = mod.torch.zeros(shape, dtype=dtype)
            _ok(z, shape, dtype)
            assert not z.view(-1).view(torch.uint8).any()
            zl = mod.torch.zeros_like(src)
            _ok(zl, shape, dtype)
            assert torch.equal(zl, torch.zeros_like(src))
            fl = mod.torch.full_like(src, 1)
            _ok(fl, shape, dtype)
            assert torch.equal(fl, src)
            fu = mod.torch.full(shape, 1, dtype=dtype)
            _ok(fu, shape, dtype)
            assert torch.equal(fu, src)
        n = len(SHAPES) * 7
        assert fz.total == n and len(fz.records) == n
        assert fz.check() == n and fz.records == []


def test_size_zero_pinned_and_cpu_pass_through(mod):
    with F.fenced("ff", (mod,), force_cpu=True) as fz:
        for t in (mod.torch.empty(0, dtype=torch.int32), mod.torch.empty((3, 0, 2)), mod.torch.zeros(0), mod.torch.zeros((0, 3)),
                  mod.torch.empty_like(torch.ones(0)), mod.torch.full((0,), 3)):
            assert t.numel() == 0 and t.storage_offset() == 0
        assert fz.total == 0
    with F.fenced("ff", (mod,)) as fz:                       # not forced: CPU tensors are left alone
        t = mod.torch.empty(9, dtype=torch.int64)
        assert t.storage_offset() == 0 and fz.total == 0
        assert mod.torch.zeros(3).storage_offset() == 0 and fz.total == 0


def test_pin_memory_passes_through(mod, monkeypatch):
    seen = []
    real = torch.empty
    monkeypatch.setattr(torch, "empty", lambda *a, **k: seen.append(k) or real(*a, **{x: y for x, y in k.items() if x != "pin_memory"}))
    fz = F.fenced("ff", (mod,), force_cpu=True)              # built after the patch: its factory wraps the recorder above
    with fz:
        t = mod.torch.empty(8, dtype=torch.int64, pin_memory=True)
    assert t.storage_offset() == 0 and fz.total == 0 and seen == [{"dtype": torch.int64, "pin_memory": True}]


@pytest.mark.parametrize("dtype", DTYPES)
def test_poisons(mod, dtype):
    shape = (3, 1001)
    with F.fenced("ff", (mod,), force_cpu=True):
        t = mod.torch.empty(shape, dtype=dtype)
        assert bool((t.view(-1).view(torch.uint8) == 0xFF).all())
        if dtype.is_floating_point:
            assert bool(torch.isnan(t).all())
        elif dtype not in (torch.bool, torch.uint8):
            assert bool((t == -1).all())
        assert bool((mod.torch.empty_like(t).view(-1).view(torch.uint8) == 0xFF).all())
    with F.fenced("zero", (mod,), force_cpu=True):
        assert not mod.torch.empty(shape, dtype=dtype).view(-1).view(torch.uint8).any()
    got = []
    for seed in (5, 5, 6):
        with F.fenced("rand", (mod,), seed=seed, force_cpu=True):
            got.append(mod.torch.empty(shape, dtype=dtype).view(-1).view(torch.uint8).numpy().copy())
    ref = np.random.default_rng(5).integers(0, 256, F._RAND_POOL, dtype=np.uint8)
    assert np.array_equal(got[0], got[1]) and not np.array_equal(got[0], got[2])
    assert np.array_equal(got[0], np.resize(ref, got[0].size)) and len(np.unique(got[0])) > 200


def test_rand_poison_repeats_over_long_payloads(mod):
    n = 2 * F._RAND_POOL + 77
    with F.fenced("rand", (mod,), seed=1, force_cpu=True):
        t = mod.torch.empty(n, dtype=torch.uint8).numpy()
    assert np.array_equal(t, np.resize(np.random.default_rng(1).integers(0, 256, F._RAND_POOL, dtype=np.uint8), n))


def test_value_factories_are_not_poisoned(mod):
    with F.fenced("ff", (mod,), force_cpu=True) as fz:
        assert torch.equal(mod.torch.full((5,), -1, dtype=torch.int32), torch.full((5,), -1, dtype=torch.int32))
        assert torch.equal(mod.torch.ones(4, dtype=torch.int64), torch.ones(4, dtype=torch.int64))
        assert torch.equal(mod.torch.arange(7, dtype=torch.int64), torch.arange(7))
        assert torch.equal(mod.torch.tensor([[1.5, 2.0]], dtype=torch.float32), torch.tensor([[1.5, 2.0]]))
        assert fz.total == 4
        fz.check()


def _alloc_here(mod, n=100, dtype=torch.int32):
    return mod.torch.empty(n, dtype=dtype)            # <- the call site the reports must name


ALLOC_LINE = _alloc_here.__code__.co_firstlineno + 1


# byte offsets relative to the payload: -1 is the byte in front of it, nbytes the first byte behind it
@pytest.mark.parametrize("where,side,first", [(-1, "left", 1), (-F.FENCE, "left", F.FENCE), (-2000, "left", 2000),
                                              ("end", "right", 1), ("gap_end", "right", 112), ("fence0", "right", 113),
                                              ("last", "right", 112 + F.FENCE)])
def test_one_byte_breach_is_reported(mod, where, side, first):
    with F.fenced("ff", (mod,), force_cpu=True) as fz:
        other = mod.torch.zeros(3)
        t = _alloc_here(mod)                               # 400 bytes: the gap to 512 is 112 bytes and counts as right fence
        rec = fz.records[-1]
        assert rec.nbytes == 400 and rec.base.numel() == F.FENCE + 512 + F.FENCE
        pos = {"end": 400, "gap_end": 511, "fence0": 512, "last": 512 + F.FENCE - 1}.get(where, where)
        rec.base[rec.off + pos] = 0
        with pytest.raises(F.FenceBreach) as e:
            fz.check()
        assert len(e.value.breaches) == 1
        r, s, a, b = e.value.breaches[0]
        assert r is rec and s == side and a == b == first
        msg = str(e.value)
        assert "test_fenced_cpu.py:%d" % ALLOC_LINE in msg and side + " fence" in msg and "(100,)" in msg and "int32" in msg
        assert fz.records == [] and other is not None      # check() dropped the records
        assert fz.check() == 0


def test_breach_span_and_several_allocations(mod):
    with F.fenced("zero", (mod,), force_cpu=True) as fz:
        a, b, c = _alloc_here(mod, 128), mod.torch.zeros(64, dtype=torch.float64), _alloc_here(mod, 3, torch.int16)
        ra, rb, rc = fz.records
        ra.base[ra.off + ra.nbytes + 8:ra.off + ra.nbytes + 24] = 1      # 16 bytes, 8 past the payload (512 bytes: no gap)
        rc.base[rc.off - 4:rc.off] = 7
        rc.base[rc.off + rc.nbytes] = 7
        with pytest.raises(F.FenceBreach) as e:
            fz.check()
        assert [(x[0], x[1], x[2], x[3]) for x in e.value.breaches] == [(ra, "right", 9, 24), (rc, "left", 1, 4), (rc, "right", 1, 1)]
        assert "zeros" not in str(e.value).split("\n", 1)[1]


def test_payload_writes_are_not_breaches(mod):
    with F.fenced("ff", (mod,), force_cpu=True) as fz:
        for dtype in DTYPES:
            t = mod.torch.empty(101, dtype=dtype)
            t.view(-1).view(torch.uint8)[-1] = 3           # the last payload byte
            t.view(-1).view(torch.uint8)[0] = 3            # and the first
            t.zero_()
        assert fz.check() == len(DTYPES)


def test_threads_are_both_recorded(mod):
    with F.fenced("rand", (mod,), force_cpu=True) as fz:
        def work(k):
            for i in range(50):
                mod.torch.empty(10 + k, dtype=torch.int32)
        ts = [threading.Thread(target=work, args=(k,)) for k in (0, 1)]
        [t.start() for t in ts]
        [t.join() for t in ts]
        assert fz.total == 100
        assert sorted(r.shape for r in fz.records) == [(10,)] * 50 + [(11,)] * 50
        assert fz.check() == 100


def test_proxy_leaves_everything_else_reachable(mod):
    with F.fenced("ff", (mod,), force_cpu=True) as fz:
        p = mod.torch
        assert p is fz.proxy and p is not torch
        assert p.cuda is torch.cuda and p.from_numpy is torch.from_numpy and p.int64 is torch.int64 and p.Tensor is torch.Tensor
        assert p.cat is torch.cat and p.device is torch.device and p.distributed is torch.distributed
        assert isinstance(p.empty(2), p.Tensor)
        assert torch.equal(p.from_numpy(np.arange(3)), torch.arange(3))
        with pytest.raises(AttributeError):
            p.no_such_thing
        for name in F.FACTORIES:
            assert getattr(p, name) is not getattr(torch, name)


def test_modules_are_restored_also_after_an_exception(mod):
    other = _module()
    with F.fenced("ff", (mod, other)):
        assert mod.torch is not torch and other.torch is not torch
    assert mod.torch is torch and other.torch is torch
    with pytest.raises(ZeroDivisionError):
        with F.fenced("ff", (mod, other)):
            1 / 0
    assert mod.torch is torch and other.torch is torch
    fz = F.fenced("ff", (mod, other)).install()               # by hand: child processes and rank threads
    assert mod.torch is fz.proxy
    with pytest.raises(RuntimeError):
        fz.install()
    fz.uninstall()
    assert mod.torch is torch and other.torch is torch
    broken = types.ModuleType("no_torch_here")
    with pytest.raises(RuntimeError):
        F.fenced("ff", (mod, broken)).install()
    assert mod.torch is torch                                  # a failed install leaves nothing behind
    with pytest.raises(ValueError):
        F.fenced("nan", (mod,))


def test_package_modules_are_restored():
    mods = F.package_modules()
    assert len(mods) >= 4
    with F.fenced("ff", mods) as fz:
        assert all(m.torch is fz.proxy for m in mods)
    assert all(m.torch is torch for m in mods)


def test_package_factories_are_all_known():
    """Every torch.<factory>( the package calls is either fenced or a known operator on existing tensors."""
    import re
    known = set(F.FACTORIES) | {"from_numpy", "cat", "stack", "device", "is_tensor", "equal", "as_tensor", "aminmax"}
    pkg = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tomography_3d_reconstructor_amd")
    used = set()
    for fn in os.listdir(pkg):
        if fn.endswith(".py"):
            used |= set(re.findall(r"\btorch\.([a-z_]+)\(", open(os.path.join(pkg, fn)).read()))
    assert used <= known, sorted(used - known)


def test_unchanged(mod):
    fz = F.fenced("ff", (mod,))
    a, b = torch.arange(10, dtype=torch.float32), torch.ones((3, 4), dtype=torch.bool)
    with fz.unchanged(a, b):
        a.clone().add_(1)
    with pytest.raises(AssertionError, match="input tensor 1"):
        with fz.unchanged(a, b):
            b[2, 3] = False
    snap = fz.unchanged(a)
    a[0] = float("nan")                                      # NaN for a number: byte comparison, not ==
    with pytest.raises(AssertionError, match="input tensor 0"):
        snap.verify()
    n = torch.full((4,), float("nan"))
    fz.unchanged(n).verify()                                 # NaN == NaN bytewise
