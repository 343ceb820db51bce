"""The batched slot calls in one sequence on ONE context: isosurface, build and
refit share the staging buffer and each reuse their own scratch arena
(job_arena.h), smaller calls after larger ones and the other way round.  The
arenas that came later (recolor, tet, cell, surf, clip, stream, glyph,
bstream), the scratch the filters share between them and a live in-situ
engine over changing slots are test_gpu_session.py's.

Every step is checked by the slots' exported bytes against the host
restatements: spray_rt_bvh_build_device_host for built slots (of the arrays
of spray_rt_isosurface_host for extracted ones), refit_helpers' expected
boxes and records for the refit.
"""
import numpy as np
import pytest

import build_helpers as bh
import iso_helpers as ih
import refit_helpers as rh

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_LIMIT = -1, -5


def to_dev(x):
    """numpy -> GPU tensor (uint32 arrays travel as their int32 bits)."""
    import torch
    x = np.ascontiguousarray(x)
    return torch.from_numpy(x.view(np.int32) if x.dtype == np.uint32 else x).cuda()


def assert_image(c, slot, want, normals):
    got = bh.export_all(c, slot)
    assert got["NODES"] == want["nodes"].tobytes()
    assert got["TRIS"] == want["tris"].tobytes()
    assert got["PRIMS"] == want["prims"].tobytes()
    assert got["QNODES4"] == want["qnodes4"].tobytes()
    assert got["QGRID"] == want["grid"].tobytes()
    assert got["NORMALS"] == normals.tobytes()
    assert c.slot_info(slot) == {"nodes": len(want["nodes"]), "depth": want["depth"],
                                 "tris": len(want["prims"])}
    return got


def assert_isosurface(spray, c, slot, g):
    v, n, f = spray.isosurface_host(g["values"], g["origin"], g["spacing"], g["iso"])
    assert len(f) > 0
    return assert_image(c, slot, bh.build_device_host(v, f), n)


def test_one_context_through_every_batched_call(oracle):
    import torch  # noqa: F401  (one HIP runtime in the process)
    import spray_amd as spray

    mesh = {}
    for m in ("wavelet", "wavelet0", "tri1", "grid12"):
        v, f = bh.mesh(m, oracle)
        mesh[m] = (v, f, rh.vertex_colors(len(v)), rh.vertex_normals(oracle, v, f))
    c = spray.RtContext(0)
    images = {}  # slot -> its exported bytes after the last call that wrote it

    def others_unchanged(*written):
        for slot, img in images.items():
            if slot not in written:
                assert bh.export_all(c, slot) == img, slot

    # 1. two small grids, numpy fields: the first use of the iso and build arenas
    ramps = [ih.ramp_grid((5, 5, 5), 0.0, 11), ih.ramp_grid((5, 5, 5), 0.1, 12)]
    c.isosurface_domains([0, 1], ramps)
    for k in (0, 1):
        images[k] = assert_isosurface(spray, c, k, ramps[k])

    # 2. a mesh of 5,480 triangles (wavelet.ply) beside wavelet0's 1,684: more
    # scratch than the arenas' first megabyte, so the build arena grows
    vw, fw, cw, nw = mesh["wavelet"]
    v0, f0, c0, n0 = mesh["wavelet0"]
    assert len(fw) == 5480 and len(f0) == 1684
    built = bh.build_device_host(vw, fw)
    c.build_domains([2, 6], [vw, v0], [fw, f0], [cw, c0], [nw, n0])
    images[2] = assert_image(c, 2, built, nw)
    images[6] = assert_image(c, 6, bh.build_device_host(v0, f0), n0)
    others_unchanged(2, 6)

    # 3. the refit of the larger one with moved vertices, and back
    v1 = rh.deform("sin", vw)
    n1 = rh.vertex_normals(oracle, v1, fw)
    c.refit_domains([2], [v1], [n1])
    got = bh.export_all(c, 2)
    nodes = np.frombuffer(got["NODES"], rh.NODE_DTYPE)
    with np.errstate(invalid="ignore"):
        plo, phi, _ = rh.expected_boxes(built["nodes"], built["prims"], fw, v1)
    assert np.stack([nodes["l_lo"], nodes["r_lo"]], 1).tobytes() == plo.tobytes()
    assert np.stack([nodes["l_hi"], nodes["r_hi"]], 1).tobytes() == phi.tobytes()
    for k in ("left", "right"):
        assert np.array_equal(nodes[k], built["nodes"][k])
    assert got["TRIS"] == rh.expected_tris(built["prims"], fw, v1).tobytes()
    assert got["PRIMS"] == built["prims"].tobytes()
    assert got["NORMALS"] == n1.tobytes()
    assert got["QNODES4"] != images[2]["QNODES4"] and got["QGRID"] != images[2]["QGRID"]
    c.refit_domains([2], [to_dev(vw)], [to_dev(nw)])
    assert bh.export_all(c, 2) == images[2]
    others_unchanged(2)

    # a rejected call in between: a face index out of range in the second job
    vt, ft, ct, nt = mesh["tri1"]
    vg, fg, cg, ng = mesh["grid12"]
    bad = fg.copy()
    bad[7, 2] = len(vg)
    with pytest.raises(spray.SprayRtError) as e:
        c.build_domains([2, 5], [vt, vg], [ft, bad], [ct, cg], [nt, ng])
    assert e.value.code == ERR_ARG
    assert "slot 5" in str(e.value)
    others_unchanged()  # slot 2, the valid job's target, among them
    with pytest.raises(spray.SprayRtError):
        c.slot_info(5)

    # 4. two small meshes in the larger arena; host and device arrays mixed
    # inside each job
    c.build_domains([3, 4], [vt, to_dev(vg)], [to_dev(ft), fg], [ct, to_dev(cg)],
                    [to_dev(nt), ng])
    images[3] = assert_image(c, 3, bh.build_device_host(vt, ft), nt)
    images[4] = assert_image(c, 4, bh.build_device_host(vg, fg), ng)
    bh.check_queries(spray, oracle, c, 4, vg, fg, cg, ng, 21)  # colors: host and device
    bh.check_queries(spray, oracle, c, 6, v0, f0, c0, n0, 22)
    others_unchanged(3, 4)

    # an extraction whose build fails in the FIRST job, slots out of order: the
    # message names the job's index as the grid and its slot as the slot
    big = np.finfo(np.float32).max
    with pytest.raises(spray.SprayRtError) as e:
        c.isosurface_domains([7, 3], [dict(ramps[0], origin=(big, big, big)), ramps[1]])
    assert e.value.code == ERR_LIMIT
    assert "isosurface (grid 0, slot 7): build (slot 7): " in str(e.value)
    others_unchanged()
    with pytest.raises(spray.SprayRtError):
        c.slot_info(7)

    # 5. a larger grid into a loaded slot: the isosurface arena after use
    sphere = ih.grid(ih.sphere_f(ih.lattice((17, 17, 17))))
    c.isosurface_domains([0], [sphere])
    images[0] = assert_isosurface(spray, c, 0, sphere)
    others_unchanged(0)
    c.close()
