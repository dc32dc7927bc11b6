"""CPU tier of SlabJob.export_glb (one GLB from all ranks): the pure layout helper, the JSON chunk from global counts, the
argument checks of the new C entry points, and the public signatures."""
import inspect
import json

import numpy as np
import pytest

from tomography_3d_reconstructor_amd import _lib, pipeline, slab


@pytest.mark.parametrize("color_cols", [0, 3, 4])
@pytest.mark.parametrize("normals", [False, True])
def test_rank_byte_ranges_tile_the_binary_chunk(color_cols, normals):
    rng = np.random.default_rng(10 * color_cols + int(normals))
    for _ in range(50):
        world = int(rng.integers(1, 9))
        kv = [int(x) for x in rng.integers(0, 2000, world)]
        kf = [int(x) for x in rng.integers(0, 4000, world)]
        if rng.random() < 0.3:
            kv[int(rng.integers(world))] = kf[int(rng.integers(world))] = 0           # a rank without rows / without faces
        total, per = slab.glb_rank_layout(kv, kf, color_cols, normals)
        assert total == pipeline.glb_layout_bytes(sum(kv), sum(kf), color_cols, normals)
        assert len(per) == world
        names = ["POSITION", "indices"] + (["COLOR_0"] if color_cols else []) + (["NORMAL"] if normals else [])
        assert all([b[0] for b in blocks] == names for blocks in per)
        width = {"POSITION": 12, "indices": 12, "COLOR_0": 4, "NORMAL": 12}
        for r, blocks in enumerate(per):
            for name, at, nb in blocks:
                assert nb == width[name] * (kf[r] if name == "indices" else kv[r]) and at % 4 == 0
        # block after block, rank after rank inside a block: no gap, no overlap, nothing beyond the chunk
        spans = sorted((at, nb, names.index(name), r) for r, blocks in enumerate(per) for name, at, nb in blocks if nb)
        pos = 0
        for at, nb, _, _ in spans:
            assert at == pos, (at, pos)
            pos += nb
        assert pos == total
        order = [(n, r) for _, _, n, r in spans]
        assert order == sorted(order), "blocks in file order, ranks ascending inside a block"


@pytest.mark.parametrize("color_cols", [0, 3, 4])
@pytest.mark.parametrize("normals", [False, True])
def test_json_from_global_counts_is_glb_json(color_cols, normals):
    nv, nf = 1234, 2464
    minmax = np.array([-1.5, 0.25, 3.0, 7.0, 8.5, 1e3], np.float32)
    bin_len = pipeline.glb_layout_bytes(nv, nf, color_cols, normals)
    p = pipeline.GlbPacked(None, nv, nf, color_cols, bin_len, (bin_len + 7) & ~7, {}, normals)
    assert pipeline.glb_json_counts(nv, nf, color_cols, normals, minmax) == pipeline.glb_json(p, minmax)
    head, total = pipeline.glb_head(nv, nf, color_cols, normals, minmax)
    assert head[:4] == b"glTF" and int.from_bytes(head[8:12], "little") == total == len(head) + bin_len
    jl = int.from_bytes(head[12:16], "little")
    assert jl % 4 == 0 and len(head) == 20 + jl + 8 and head[16:20] == b"JSON" and head[-4:] == b"BIN\x00"
    assert int.from_bytes(head[-8:-4], "little") == bin_len
    assert json.loads(head[20:20 + jl]) == pipeline.glb_json(p, minmax)
    assert head[20:20 + jl].rstrip(b" ") == json.dumps(pipeline.glb_json(p, minmax), separators=(",", ":")).encode()
    with pytest.raises(ValueError):
        pipeline.glb_head(nv, nf, color_cols, normals, np.array([0, 0, 0, np.inf, 0, 0], np.float32))


def test_new_entry_points_check_their_arguments_without_a_gpu():
    L = _lib.lib()
    E_ARG = -1
    buf = np.zeros(4096, np.uint8)
    p = buf.ctypes.data
    assert p % 8 == 0
    # tomo_mesh_seam_edges(table, table_bytes, nf, first_ghost, msg, cap, count, stream)
    assert L.tomo_mesh_seam_edges(None, 1 << 20, 4, 0, p, 1, p, None) == E_ARG
    assert L.tomo_mesh_seam_edges(p, 1 << 20, 4, 0, p, 1, None, None) == E_ARG
    assert L.tomo_mesh_seam_edges(p, 1 << 20, 0, 0, p, 1, p, None) == E_ARG
    assert L.tomo_mesh_seam_edges(p, 1 << 20, -3, 0, p, 1, p, None) == E_ARG
    assert L.tomo_mesh_seam_edges(p, 1 << 20, 4, -1, p, 1, p, None) == E_ARG
    assert L.tomo_mesh_seam_edges(p, 1 << 20, 4, 0, p, -1, p, None) == E_ARG
    assert L.tomo_mesh_seam_edges(p, 1 << 20, 4, 0, None, 1, p, None) == E_ARG            # room for a record but no buffer
    # tomo_mesh_seam_merge(table, table_bytes, nf, msg, n, corr, stream)
    assert L.tomo_mesh_seam_merge(None, 1 << 20, 4, p, 1, p, None) == E_ARG
    assert L.tomo_mesh_seam_merge(p, 1 << 20, 4, p, 1, None, None) == E_ARG
    assert L.tomo_mesh_seam_merge(p, 1 << 20, 0, p, 1, p, None) == E_ARG
    assert L.tomo_mesh_seam_merge(p, 1 << 20, 4, p, -1, p, None) == E_ARG
    assert L.tomo_mesh_seam_merge(p, 1 << 20, 4, None, 1, p, None) == E_ARG
    # tomo_mesh_vertex_normals_seeded(pos, nv, idx, idx_i64, nf, ws, ws_bytes, normals, counters, seed, n_seed, raw, n_raw, phase, stream)
    ws = (p + 255) & ~255
    ok = dict(pos=p, nv=8, idx=p, i64=0, nf=4, ws=ws, wsb=1 << 20, nrm=p, cnt=p, seed=p, n_seed=2, raw=p, n_raw=2, phase=3)

    def seeded(**kw):
        a = dict(ok, **kw)
        return L.tomo_mesh_vertex_normals_seeded(a["pos"], a["nv"], a["idx"], a["i64"], a["nf"], a["ws"], a["wsb"], a["nrm"], a["cnt"],
                                                 a["seed"], a["n_seed"], a["raw"], a["n_raw"], a["phase"], None)
    for bad in (dict(pos=None), dict(ws=None), dict(cnt=None), dict(idx=None), dict(nrm=None), dict(seed=None), dict(raw=None),
                dict(nv=0), dict(nv=-1), dict(nf=-1), dict(n_seed=-1), dict(n_raw=-1), dict(n_raw=9), dict(n_seed=7), dict(phase=0),
                dict(phase=4), dict(ws=ws + 8)):
        assert seeded(**bad) == E_ARG, bad
    assert seeded(wsb=16) == -4                                                   # TOMO_E_WORKSPACE, still before any launch


def test_slab_job_has_the_collective_glb_export():
    sig = inspect.signature(slab.SlabJob.export_glb)
    assert list(sig.parameters) == ["self", "path", "colors", "normals", "mesh"]
    assert [sig.parameters[k].default for k in ("colors", "normals", "mesh")] == [None, False, None]
    sig = inspect.signature(slab.SlabJob.layer_colors)
    assert list(sig.parameters) == ["self", "slice_depths", "first_section1_slice", "last_section1_slice", "highlight_thickness_mm"]
    assert sig.parameters["highlight_thickness_mm"].default == 1.0
    assert "WHOLE MESH ON" in slab.SlabJob.export_glb.__doc__                     # the fallback's cost is stated
    job = slab.SlabJob(64, 8, 8, slab.ThreadComm.make(1)[0], engine=object())
    with pytest.raises(RuntimeError):
        job.export_glb("never_written.glb")
    with pytest.raises(RuntimeError):
        job.layer_colors(np.ones(64), 1, 2)
