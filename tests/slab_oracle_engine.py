"""Test-only engine for tomography_3d_reconstructor_amd.slab.SlabJob: the CPU oracle behind the engine
interface, so the Z-slab orchestration (halo exchange, close-ends stencil, global numbering) can be exercised on CPU
ranks (gloo) without a GPU.  Lives under tests/: the product never imports it."""
import numpy as np
import torch

from oracle import oracle as O


def np_pack(a):
    nz, ny, nx = a.shape
    wx = (nx + 63) // 64
    b = np.zeros((nz, ny, wx * 64), bool)
    b[:, :, :nx] = a
    return np.packbits(b, axis=2, bitorder="little").view(np.int64).reshape(nz, ny, wx)


def np_unpack(bits, shape):
    nz, ny, nx = shape
    u8 = np.ascontiguousarray(bits).view(np.uint8).reshape(nz, ny, -1)
    return np.unpackbits(u8, axis=2, bitorder="little")[:, :, :nx].astype(bool)


class OVol:
    def __init__(self, bits, shape):
        self.bits, self.shape = bits, tuple(shape)

    def arr(self):
        return np_unpack(self.bits.numpy(), self.shape)

    def set(self, a):
        self.bits.copy_(torch.from_numpy(np_pack(a)))


class OField:
    def __init__(self, data):
        self.data = data
        self.Nz, self.Ny, self.Nx = data.shape
        self.pitch, self.xorg = self.Nx, 0


class OMesh:
    def __init__(self, vpos, faces32):
        self.vpos, self.faces32 = vpos, faces32


class OracleEngine:
    def pack(self, mask):
        a = mask.numpy().astype(bool)
        return OVol(torch.from_numpy(np_pack(a)), a.shape)

    def bits(self, vol):
        return vol.bits

    def from_bits(self, bits, shape):
        return OVol(bits.contiguous().clone(), shape)

    def fill_holes(self, vol, z):
        a = vol.arr()
        if a[z].any():
            a[z] = O.fill_holes_2d(a[z])
            vol.set(a)

    def close_scan(self, vol):
        a = vol.arr()
        for z in range(1, a.shape[0] - 1):
            a[z] = a[z] | (a[z - 1] & a[z + 1])
        vol.set(a)

    def smooth(self, vol, iterations, create_manifold):
        a = O.smooth(vol.arr(), iterations, create_manifold)
        return OVol(torch.from_numpy(np_pack(a)), a.shape)

    def field(self, vol):
        return OField(torch.from_numpy(O.field(vol.arr(), True, True)))

    def field_slices(self, f, a, b):
        return OField(f.data[a:b])

    def marching_cubes(self, f, z_offset):
        try:
            v, fc = O.marching_cubes(f.data.numpy(), 0.5, z_offset)
        except (ValueError, RuntimeError):
            return None
        return OMesh(torch.from_numpy(v), torch.from_numpy(fc))

    def finalize_vertices(self, vpos, depths, mm_y, mm_x):
        out = O.finalize_vertices(vpos.numpy(), depths, mm_y, mm_x, True, True)
        vpos.copy_(torch.from_numpy(out))
        return vpos

    def unique(self, vpos):
        u, inv = np.unique(vpos.numpy(), axis=0, return_inverse=True)
        return torch.from_numpy(u), torch.from_numpy(np.asarray(inv).reshape(-1).astype(np.int32))

    def slice_counts(self, vol):
        return torch.from_numpy(vol.arr().sum(axis=(1, 2)).astype(np.int64))

    def bbox(self, vol):
        idx = np.nonzero(vol.arr())
        if len(idx[0]) == 0:
            return None
        return tuple(int(f(a)) for a in idx for f in (np.min, np.max))
