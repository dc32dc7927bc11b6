"""GPU tier of SlabJob.export_glb: ONE GLB written by all ranks together, without gathering the mesh, byte for byte the file
pipeline.export_glb writes from the gathered mesh.  Rank threads share this GPU (in-process communicator), every rank on a
stream of its own.  "Equal" below: the two files hold the same bytes and the stats dicts are equal key by key on every rank,
except signed_volume -- an atomic / tree sum on one GPU, per-rank partial sums added in rank order here -- which is compared
to 1e-6 relative, the bar DESIGN section 2 sets for the project's tree reductions."""
import os
import threading
import time

import numpy as np
import pytest
import torch

import glb_normals_reference as N
from tomography_3d_reconstructor_amd import pipeline, slab

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def blob(nz, ny, nx, scale, seed):
    rng = np.random.default_rng(seed)
    zz, yy, xx = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    v = ((zz - nz / 2) / (nz * 0.48 * scale)) ** 2 + ((yy - ny / 2) / (ny * 0.42 * scale)) ** 2 + ((xx - nx / 2) / (nx * 0.45 * scale)) ** 2 <= 1
    v ^= rng.random(v.shape) < 0.004
    return v


def ellipsoid(nz, ny, nx):
    zz, yy, xx = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    return ((zz - (nz - 1) / 2) / (0.45 * nz)) ** 2 + ((yy - (ny - 1) / 2) / (0.40 * ny)) ** 2 + ((xx - (nx - 1) / 2) / (0.42 * nx)) ** 2 <= 1


def on_ranks(comms, fn, timeout=300):
    """fn(comm) on one thread per rank, each on its own stream -> the ranks' results; no thread may be left waiting."""
    world = len(comms)
    out, errs = [None] * world, []

    def target(c):
        try:
            with torch.cuda.stream(torch.cuda.Stream()):
                out[c.rank] = fn(c)
                torch.cuda.current_stream().synchronize()
        except BaseException as e:   # noqa: BLE001
            errs.append(e)
            raise

    ts = [threading.Thread(target=target, args=(c,)) for c in comms]
    [t.start() for t in ts]
    [t.join(timeout) for t in ts]
    assert not any(t.is_alive() for t in ts), "a rank is still waiting in a collective step"
    assert not errs, errs
    torch.cuda.synchronize()
    return out


def run_jobs(dev, mask, depths, world, z_cuts=None, mm=(1.0, 1.0)):
    """One pass of a SlabJob per rank thread over `mask` (device, (nz, ny, nx)) -> (comms, jobs)."""
    nz, ny, nx = mask.shape
    comms = slab.ThreadComm.make(world)

    def one(c):
        job = slab.SlabJob(nz, ny, nx, c, z_cuts=z_cuts)
        job.run(mask[job.z0:job.z1].view(torch.uint8), depths, mm[0], mm[1])
        return job
    return comms, on_ranks(comms, one)


def names_a_ghost_row(jobs, meshes):
    """At least one face of a rank below the top one names a row of the rank above: the seam is really exercised."""
    return any(m[1].shape[0] and int(m[1].max().item()) >= j.vertex_offset + m[0].shape[0] for j, m in zip(jobs[:-1], meshes[:-1]))


def same_stats(got, exp):
    assert set(got) == set(exp), (sorted(got), sorted(exp))
    for key in exp:
        if key == "signed_volume":
            assert abs(got[key] - exp[key]) <= 1e-6 * abs(exp[key]), (got[key], exp[key])
        else:
            assert got[key] == exp[key] and type(got[key]) is type(exp[key]), (key, got[key], exp[key])


def same_file(a, b):
    assert os.path.getsize(a) == os.path.getsize(b), (os.path.getsize(a), os.path.getsize(b))
    with open(a, "rb") as fa, open(b, "rb") as fb:
        at = 0
        while True:
            ca, cb = fa.read(1 << 26), fb.read(1 << 26)
            if ca != cb:
                x, y = np.frombuffer(ca, np.uint8), np.frombuffer(cb, np.uint8)
                raise AssertionError("the slab job's GLB differs from the single-GPU export at byte %d" % (at + int(np.flatnonzero(x != y)[0])))
            if not ca:
                return
            at += len(ca)


def export_both(dev, comms, jobs, tmp_path, colors=None, normals=False, meshes=None, tag="x"):
    """The collective export next to pipeline.export_glb of the gathered mesh -> (single-GPU stats, per-rank stats, paths)."""
    meshes = [j.mesh for j in jobs] if meshes is None else meshes
    many, single = str(tmp_path / (tag + "_ranks.glb")), str(tmp_path / (tag + "_single.glb"))
    stats = on_ranks(comms, lambda c: jobs[c.rank].export_glb(many, colors=None if colors is None else colors[c.rank], normals=normals,
                                                              mesh=meshes[c.rank]))
    V, F = torch.cat([m[0] for m in meshes]), torch.cat([m[1] for m in meshes])
    C = None if colors is None else torch.cat(list(colors))
    exp = pipeline.export_glb(single, V, F, C, normals)
    return exp, stats, many, single, (V, F)


def check_equal(exp, stats, many, single):
    same_file(many, single)
    for s in stats:
        same_stats(s, exp)


CASES = {
    # name: (volume, depths, world, z_cuts)
    "blob2": (lambda: blob(128, 96, 144, 1.0, 5), lambda nz: np.concatenate([np.full(40, 0.5), np.full(48, 0.25), np.full(40, 0.75)]), 2, None),
    "blob3": (lambda: blob(128, 96, 144, 1.0, 5), lambda nz: np.full(nz, 0.4), 3, None),
    "blob4": (lambda: blob(128, 96, 144, 1.0, 6), lambda nz: np.full(nz, 0.4), 4, None),
    "thin3": (lambda: ellipsoid(320, 64, 80), lambda nz: np.full(nz, 0.5), 3, [0, 140, 190, 320]),      # unequal cuts, one slab of 50 slices
    "empty3": (lambda: np.concatenate([blob(72, 96, 112, 1.0, 3), np.zeros((48, 96, 112), bool)]), lambda nz: np.full(nz, 0.4), 3, None),
}


@pytest.mark.parametrize("case,colour,normals", [
    ("blob2", None, False), ("blob2", "layer", True), ("blob3", "rgb", True), ("blob3", "layer", False), ("blob4", None, True),
    ("blob4", "layer", True), ("thin3", "layer", True), ("thin3", None, False), ("empty3", "layer", True), ("empty3", "rgb", False)])
def test_job_meshes(dev, tmp_path, case, colour, normals):
    make, make_depths, world, cuts = CASES[case]
    vol = make()
    nz = vol.shape[0]
    depths = make_depths(nz)
    mask = torch.from_numpy(np.ascontiguousarray(vol).view(np.uint8)).to(dev)
    comms, jobs = run_jobs(dev, mask, depths, world, cuts, (0.7, 0.9))
    if case == "thin3":
        assert min(j.z1 - j.z0 for j in jobs) < 128 <= max(j.z1 - j.z0 for j in jobs)
    if case == "empty3":
        assert jobs[2].mesh[0].shape[0] == 0 and jobs[2].mesh[1].shape[0] == 0, "the top slab was meant to be empty"
    assert names_a_ghost_row(jobs, [j.mesh for j in jobs])
    colors = None
    if colour:
        first, last = nz // 8, nz // 2
        colors = on_ranks(comms, lambda c: jobs[c.rank].layer_colors(depths, first, last, 1.5))
        whole = pipeline.layer_colors(torch.cat([j.mesh[0] for j in jobs]), depths, first, last, 1.5)
        assert torch.equal(torch.cat(colors), whole) and all(c.shape == (j.mesh[0].shape[0], 4) for c, j in zip(colors, jobs))
        assert len(torch.unique(whole[:, :3], dim=0)) == 3, "the stack was meant to show all three layer colours"
        if colour == "rgb":
            colors = [c[:, :3].contiguous() for c in colors]
    exp, stats, many, single, _ = export_both(dev, comms, jobs, tmp_path, colors, normals)
    assert exp["fast_path"] is True and all(s["fast_path"] is True for s in stats)
    assert exp["boundary_edges"] == 0 and exp["inconsistent_pairs"] == 0
    check_equal(exp, stats, many, single)
    assert all(j.glb_last["bytes_sent"] is not None for j in jobs), "the distributed path was meant to run"


def normal_block(path, nv):
    data = open(path, "rb").read()
    jl = int.from_bytes(data[12:16], "little")
    binc = data[20 + jl + 8:]
    return np.frombuffer(binc[len(binc) - 12 * nv:], np.float32).reshape(nv, 3)


def index_block(path, nv, nf):
    data = open(path, "rb").read()
    jl = int.from_bytes(data[12:16], "little")
    return np.frombuffer(data[20 + jl + 8 + 12 * nv:20 + jl + 8 + 12 * nv + 12 * nf], np.uint32).reshape(nf, 3).astype(np.int64)


def test_normals_across_the_seam_against_the_restated_contract(dev, tmp_path):
    """Three ranks: the NORMAL block of the jointly written file against tests/glb_normals_reference.py on the gathered mesh
    (positions as stored, the oriented faces the file stores), so that the two GPU paths cannot be wrong in the same way."""
    vol = blob(128, 96, 144, 1.0, 5)
    depths = np.full(128, 0.4)
    mask = torch.from_numpy(np.ascontiguousarray(vol).view(np.uint8)).to(dev)
    comms, jobs = run_jobs(dev, mask, depths, 3, None, (0.7, 0.9))
    assert names_a_ghost_row(jobs, [j.mesh for j in jobs])
    exp, stats, many, single, (V, F) = export_both(dev, comms, jobs, tmp_path, None, True)
    check_equal(exp, stats, many, single)
    nv, nf = V.shape[0], F.shape[0]
    oriented = index_block(many, nv, nf)
    ref, defaulted = N.vertex_normals(V.cpu().numpy(), oriented)
    got = normal_block(many, nv)
    assert got.tobytes() == ref.tobytes()
    assert all(s["normals_defaulted"] == defaulted for s in stats)
    # rows on the shared planes: named by faces of two ranks
    shared = sum(int(((m[1] >= j.vertex_offset + m[0].shape[0]).any(1)).sum().item()) for j, m in zip(jobs[:-1], [j.mesh for j in jobs[:-1]]))
    assert shared > 0


def bipyramid_chain(world, n, seed=2):
    """A hand-built mesh for `world` ranks in the job's layout.  A marching-cubes vertex has 4 to 9 faces (at most 12 on this
    lattice), so the generator cannot make a shared-plane vertex with more than 16: here rank j holds a bipyramid over a ring
    of n vertices whose upper apex is the FIRST row of rank j + 1 (a ghost row of rank j, the hub) and whose lower apex is
    its own first row -- the hub of the rank below.  A hub has n faces on the lower rank and n on the upper one: with n > 16
    the lower rank's raw sums and the owner's seeded continuation both take the long-list path.  Faces are shuffled inside
    a rank.  -> per rank (vertices float32, faces int64 with global indices), offsets."""
    rng = np.random.default_rng(seed)
    rows, offs = [], [0]
    for j in range(world):
        a = np.arange(n) * 2 * np.pi / n + 0.1 * j
        rad = 1.0 + 0.3 * np.sin(3 * a + j) + 0.05 * rng.random(n)
        ring = np.stack([np.full(n, 2.0 * j + 1.0) + 0.2 * np.cos(2 * a), rad * np.cos(a), rad * np.sin(a)], 1)
        low = np.array([[2.0 * j + (0.0 if j == 0 else 0.013 * j), 0.07 * j, -0.05 * j]])
        own = [low, ring] + ([np.array([[2.0 * world, 0.1, 0.2]])] if j == world - 1 else [])
        rows.append(np.concatenate(own).astype(np.float32))
        offs.append(offs[-1] + len(rows[-1]))
    meshes = []
    for j in range(world):
        lo = offs[j]
        ring = offs[j] + 1 + np.arange(n)
        hi = offs[j + 1] if j + 1 < world else offs[j] + 1 + n
        nxt = np.roll(ring, -1)
        f = np.concatenate([np.stack([np.full(n, lo), nxt, ring], 1), np.stack([np.full(n, hi), ring, nxt], 1)])
        meshes.append((rows[j], f[rng.permutation(len(f))].astype(np.int64)))
    return meshes, offs


@pytest.mark.parametrize("n", [40, 9])
def test_long_lists_on_a_shared_row_through_a_hand_built_mesh(dev, tmp_path, n):
    world = 3
    host, offs = bipyramid_chain(world, n)
    comms = slab.ThreadComm.make(world)
    jobs = []
    for c in comms:
        job = slab.SlabJob(64 * world, 16, 16, c)
        job.vertex_offset, job.n_vertices_global = offs[c.rank], offs[-1]       # the numbering run() would have published
        jobs.append(job)
    meshes = [(torch.from_numpy(v).to(dev), torch.from_numpy(f).to(dev)) for v, f in host]
    assert names_a_ghost_row(jobs, meshes)
    exp, stats, many, single, (V, F) = export_both(dev, comms, jobs, tmp_path, None, True, meshes, "chain%d" % n)
    assert exp["fast_path"] is True
    check_equal(exp, stats, many, single)
    deg = np.bincount(F.cpu().numpy().reshape(-1), minlength=V.shape[0])
    assert [int(deg[offs[j]]) for j in (1, 2)] == [2 * n, 2 * n]                # the hubs: n faces below, n above
    ref, defaulted = N.vertex_normals(V.cpu().numpy(), index_block(many, V.shape[0], F.shape[0]))
    assert normal_block(many, V.shape[0]).tobytes() == ref.tobytes() and defaulted == 0


def seam_setup(dev):
    vol = blob(128, 96, 144, 1.0, 5)
    depths = np.full(128, 0.4)
    mask = torch.from_numpy(np.ascontiguousarray(vol).view(np.uint8)).to(dev)
    comms, jobs = run_jobs(dev, mask, depths, 2, None, (0.7, 0.9))
    meshes = [j.mesh for j in jobs]
    assert names_a_ghost_row(jobs, meshes)
    off1 = jobs[1].vertex_offset
    n_ghost = int(meshes[0][1].max().item()) - off1 + 1
    return comms, jobs, meshes, off1, n_ghost


@pytest.mark.parametrize("side", ["upper", "lower"])
def test_seam_bookkeeping_on_an_open_mesh(dev, tmp_path, side):
    """Faces that touch the shared plane are dropped from one rank: boundary edges now pair across the ranks."""
    comms, jobs, meshes, off1, n_ghost = seam_setup(dev)
    v0, f0 = meshes[0]
    v1, f1 = meshes[1]
    if side == "upper":
        touch = torch.nonzero((f1 < off1 + n_ghost).any(1)).reshape(-1)          # faces of rank 1 that name a shared-plane row
        keep = torch.ones(f1.shape[0], dtype=torch.bool, device=dev)
        keep[touch[::5][:7]] = False
        edited = [(v0, f0), (v1, f1[keep].contiguous())]
    else:
        touch = torch.nonzero((f0 >= off1).any(1)).reshape(-1)                   # faces of rank 0 that name a ghost row
        keep = torch.ones(f0.shape[0], dtype=torch.bool, device=dev)
        keep[touch[::5][:7]] = False
        edited = [(v0, f0[keep].contiguous()), (v1, f1)]
    assert len(touch) >= 35
    exp, stats, many, single, _ = export_both(dev, comms, jobs, tmp_path, None, True, edited, side)
    assert exp["boundary_edges"] > 0 and exp["fast_path"] is True
    check_equal(exp, stats, many, single)
    assert all(j.glb_last["bytes_sent"] is not None for j in jobs)


def test_fallback_when_the_winding_is_not_consistent(dev, tmp_path):
    """Every seventh face reversed on every rank: the union-find has to run, on the whole mesh, on rank 0."""
    comms, jobs, meshes, _, _ = seam_setup(dev)
    edited = []
    for v, f in meshes:
        f = f.clone()
        f[::7] = f[::7].flip(1)
        edited.append((v, f))
    first = jobs[0].layer_colors(np.full(128, 0.4), 30, 90)                      # (rank 0's own rows; one thread suffices here)
    colors = [first, jobs[1].layer_colors(np.full(128, 0.4), 30, 90)]
    torch.cuda.synchronize()
    exp, stats, many, single, _ = export_both(dev, comms, jobs, tmp_path, colors, True, edited, "flipped")
    assert exp["inconsistent_pairs"] > 0 and exp["fast_path"] is False and exp["components"] is not None
    check_equal(exp, stats, many, single)
    assert all(j.glb_last.get("gathered") for j in jobs)


def test_a_failure_on_one_rank_is_raised_on_every_rank(dev, tmp_path):
    comms, jobs, meshes, _, _ = seam_setup(dev)
    world = len(jobs)
    raised = [[None, None] for _ in range(world)]
    short = str(tmp_path / "short.glb")
    bad_path = str(tmp_path / "no_such_directory" / "slab.glb")
    good = str(tmp_path / "good.glb")

    def one(c):
        job = jobs[c.rank]
        k = job.mesh[0].shape[0]
        col = torch.zeros((k - 1 if c.rank == 1 else k, 4), dtype=torch.uint8, device=dev)      # one row short on rank 1 alone
        try:
            job.export_glb(short, colors=col)
        except Exception as e:   # noqa: BLE001
            raised[c.rank][0] = e
        try:
            job.export_glb(bad_path, normals=True)
        except Exception as e:   # noqa: BLE001
            raised[c.rank][1] = e
        return job.export_glb(good, normals=True)            # the job is still usable

    stats = on_ranks(comms, one, timeout=120)
    assert all(type(r[0]) is ValueError for r in raised), raised
    assert all(type(r[1]) is OSError and "creating the file" in str(r[1]) for r in raised), raised
    assert not os.path.exists(short) and not os.path.exists(bad_path)
    assert os.path.getsize(good) > 0 and stats[0] == stats[1]


def test_one_rank_delegates_to_the_single_gpu_export(dev, tmp_path):
    vol = blob(64, 48, 80, 1.0, 4)
    depths = np.full(64, 0.5)
    mask = torch.from_numpy(np.ascontiguousarray(vol).view(np.uint8)).to(dev)
    comms, jobs = run_jobs(dev, mask, depths, 1)
    colors = [jobs[0].layer_colors(depths, 10, 40)]
    exp, stats, many, single, _ = export_both(dev, comms, jobs, tmp_path, colors, True)
    check_equal(exp, stats, many, single)


def test_full_size_config_with_four_ranks(dev, tmp_path):
    """BASELINE configs[3], the 1024 x 1024 x 2048 ellipsoid: four rank threads, colours and normals on; the file equals the
    single-GPU export of the same mesh.  The times printed are measurements (four threads share one card and one file
    system): nothing is asserted about them."""
    nz, ny, nx = 2048, 1024, 1024
    mask = pipeline.ellipsoid_mask(nz, ny, nx, dev)
    depths = np.full(nz, 1.0)
    comms, jobs = run_jobs(dev, mask, depths, 4)
    del mask
    assert names_a_ghost_row(jobs, [j.mesh for j in jobs])
    colors = on_ranks(comms, lambda c: jobs[c.rank].layer_colors(depths, 512, 1536, 8.0))
    many, single = str(tmp_path / "cfg4_ranks.glb"), str(tmp_path / "cfg4_single.glb")
    try:
        timing = [None] * 4

        def one(c):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            a.record()
            s = jobs[c.rank].export_glb(many, colors=colors[c.rank], normals=True)
            b.record()
            b.synchronize()
            timing[c.rank] = (time.perf_counter() - t0, a.elapsed_time(b))
            return s
        stats = on_ranks(comms, one, timeout=900)
        V, F, C = torch.cat([j.mesh[0] for j in jobs]), torch.cat([j.mesh[1] for j in jobs]), torch.cat(colors)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        exp = pipeline.export_glb(single, V, F, C, True)
        t_single = time.perf_counter() - t0
        print("cfg4 slab glb: %d vertices, %d faces, %d bytes; single-GPU export %.1f ms host to host; ranks (host s, stream ms) %s; sent %s" % (
            V.shape[0], F.shape[0], os.path.getsize(single), 1e3 * t_single, [(round(h, 4), round(d, 2)) for h, d in timing],
            [j.glb_last for j in jobs]))
        assert exp["fast_path"] is True
        check_equal(exp, stats, many, single)
    finally:
        for p in (many, single):
            if os.path.exists(p):
                os.remove(p)
