"""Isosurfaces of tetrahedral meshes on the GPU (spray_rt_tet_isosurface,
spray_rt_domains_tet_isosurface).

References, each bit for bit: the host restatement
(spray_rt_tet_isosurface_host, itself checked against numpy and against the
structured extraction in test_tet_isosurface_host.py) for the extracted arrays,
a build_domains of the restated arrays in a second context for the slot images,
an upload of the same meshes for the scene launch, the oracle's brute force for
queries.
"""
import numpy as np
import pytest

import build_helpers as bh
import refit_helpers as rh
import tet_helpers as th

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_LIMIT = -1, -5
WHAT = bh.WHAT + ("COLORS", "FACES")
KEPT = tuple(w for w in WHAT if w != "COLORS")
F32 = np.float32


@pytest.fixture(scope="module")
def spray():
    import torch  # noqa: F401  (one HIP runtime in the process)
    import spray_amd
    return spray_amd


@pytest.fixture(scope="module")
def meshes():
    return th.gpu_meshes()


@pytest.fixture(scope="module")
def restated(spray, meshes):
    """(verts, normals, colors, faces) of every mesh from the host restatement."""
    return [th.host_mesh(spray, m) for m in meshes]


def slot_colors(m, col):
    """The colour array a slot of mesh m carries: none without a field or a colour."""
    return col if m.get("cfield") is not None or m.get("color") is not None else None


def export_all(c, slot, what=WHAT):
    return {w: c.slot_export(slot, getattr(c, "SLOT_" + w)).tobytes() for w in what}


def synced(c, x):
    """x once the context's stream has run: the calls are enqueued there, and
    torch reads on another stream."""
    c.sync()
    return x


def as_bytes(mesh):
    return tuple(None if x is None else x.cpu().numpy().tobytes() for x in mesh)


def ref_bytes(mesh):
    return tuple(None if x is None else x.tobytes() for x in mesh)


def test_batch_shapes(meshes, restated):
    """The meshes reach the paths they are there for."""
    nt = [len(m["tets"]) for m in meshes]
    assert nt[th.SINGLE] == 1 and nt[th.CUBE] == 5
    assert nt[th.FULL] == 3840 == 15 * 256                  # the last block full
    assert nt[th.PARTIAL] % 256 != 0 and nt[th.PARTIAL] > 256   # a partial last block
    assert nt[th.LARGE] == 131712 and -(-nt[th.LARGE] // 256) == 515 > 512   # past one scan stride
    assert th.instances(meshes[th.LARGE]) > 512 * 256       # ... of the second scan too
    assert len(restated[th.EMPTY][0]) == 0 and 0 < th.EMPTY < len(meshes) - 1
    for k in (th.SINGLE, th.CUBE, th.SMALL, th.FULL, th.PARTIAL, th.LARGE, th.REORIENTED):
        assert len(restated[k][3]) > 0, k
    assert [m.get("cfield") is not None for m in meshes] == [False, False, True, True, False, True,
                                                            True, True]
    assert meshes[th.SMALL]["cmap"][0].size == 1 and meshes[th.FULL]["cmap"][0].size == 4096
    assert meshes[th.SINGLE].get("color") is None and meshes[th.CUBE]["color"] is not None
    assert [m.get("normals") is not None for m in meshes] == [False, True, False, True, True, True,
                                                             True, True]
    tab = meshes[th.FULL]["cmap"][0]                        # both ends of a clamped range
    assert {int(tab[0]), int(tab[-1])} <= set(restated[th.FULL][2].tolist())
    assert len(np.unique(restated[th.LARGE][2])) > 8


@pytest.mark.parametrize("device", [True, False], ids=["tensors", "numpy"])
def test_kernels_equal_the_host_restatement(spray, meshes, restated, device):
    c = spray.RtContext(0)
    ms = th.on_device(meshes) if device else meshes
    got = [as_bytes(m) for m in synced(c, c.tet_isosurface(ms))]
    for k, ref in enumerate(restated):
        assert got[k] == ref_bytes(ref), k
    # the same batch in reversed order, without normals: the same bytes per mesh
    rev = [as_bytes(m) for m in synced(c, c.tet_isosurface(ms[::-1], normals=False))][::-1]
    for k in range(len(meshes)):
        assert rev[k] == (got[k][0], None, got[k][2], got[k][3]), k
    # twice: the same bytes
    again = [as_bytes(m) for m in synced(c, c.tet_isosurface(ms))]
    assert again == got
    c.close()


def test_count_only_form(spray, meshes, restated):
    c = spray.RtContext(0)
    want = [(len(r[0]), len(r[3])) for r in restated]
    assert c.tet_isosurface(th.on_device(meshes), count_only=True) == want
    assert c.tet_isosurface(meshes, count_only=True) == want
    assert c.tet_isosurface([], count_only=True) == []
    c.close()


def test_phase_times(spray, meshes, restated):
    c = spray.RtContext(0)
    ms = th.on_device([meshes[th.FULL], meshes[th.PARTIAL]])
    c.tet_isosurface(ms, count_only=True)
    t = c.tet_phase_times()
    assert t[0] > 0 and t[1] > 0 and t[2] == 0 and t[3] == 0   # no emit, timing off
    c.tet_phase_times(on=True)
    got = synced(c, c.tet_isosurface(ms, capacity=(len(restated[th.FULL][0]),
                                                   len(restated[th.FULL][3]))))
    t = c.tet_phase_times(on=False)
    assert all(x > 0 for x in t) and t[3] < t[1]               # the sort runs inside phase 2
    assert as_bytes(got[0]) == ref_bytes(restated[th.FULL])    # timing changes no byte
    c.close()


def test_short_capacities_write_nothing(spray, meshes, restated):
    c = spray.RtContext(0)
    ms = th.on_device([meshes[th.CUBE], meshes[th.FULL]])
    nv, nf = len(restated[th.FULL][0]), len(restated[th.FULL][3])
    counts = [(len(restated[k][0]), len(restated[k][3])) for k in (th.CUBE, th.FULL)]
    for cap in ((nv - 1, nf), (nv, nf - 1)):
        with pytest.raises(spray.SprayRtError) as e:
            c.tet_isosurface(ms, capacity=cap)
        assert e.value.code == ERR_LIMIT and "mesh 1" in str(e.value)
        assert e.value.counts == counts
        c.sync()
        for bufs in e.value.buffers:   # zeroed before the call: untouched
            assert all(int(b.abs().max()) == 0 for b in bufs)
    # the exact capacities fit
    got = synced(c, c.tet_isosurface(ms, capacity=(nv, nf)))
    assert as_bytes(got[1]) == ref_bytes(restated[th.FULL])
    assert as_bytes(got[0]) == ref_bytes(restated[th.CUBE])
    c.close()


def test_slot_images_equal_a_build_of_the_restated_arrays(spray, meshes, restated):
    n = len(meshes)
    c, B = spray.RtContext(0), spray.RtContext(0)
    bounds = c.tet_isosurface_domains(list(range(n)), th.on_device(meshes), bounds=True)
    cols = [slot_colors(m, r[2]) for m, r in zip(meshes, restated)]
    ref_bounds = B.build_domains(list(range(n)), [r[0] for r in restated],
                                 [r[3] for r in restated], cols, [r[1] for r in restated],
                                 bounds=True)
    for k in range(n):
        assert export_all(c, k) == export_all(B, k), k
        assert c.slot_info(k) == B.slot_info(k)
        assert c.slot_export(k, c.SLOT_FACES).tobytes() == restated[k][3].tobytes()
        got = c.slot_export(k, c.SLOT_COLORS)
        assert got.tobytes() == (b"" if cols[k] is None else cols[k].tobytes()), k
    assert bounds.tobytes() == ref_bounds.tobytes()
    # numpy arrays, other slots, no normals
    pick = (th.FULL, th.SINGLE)
    c.tet_isosurface_domains([9, 8], [meshes[k] for k in pick], normals=False)
    B.build_domains([9, 8], [restated[k][0] for k in pick], [restated[k][3] for k in pick],
                    [cols[k] for k in pick])
    for k in (9, 8):
        assert export_all(c, k) == export_all(B, k), k
    c.close()
    B.close()


def test_queries_equal_the_brute_force(spray, oracle, meshes, restated):
    c = spray.RtContext(0)
    c.tet_isosurface_domains([3, 1], th.on_device([meshes[th.FULL], meshes[th.PARTIAL]]))
    for slot, k, seed in ((3, th.FULL, 71), (1, th.PARTIAL, 72)):
        v, n, col, f = restated[k]
        bh.check_queries(spray, oracle, c, slot, v, f, col, n, seed)
    c.close()


def test_scene_launches_equal_uploaded_slots(spray, oracle, meshes):
    ma = meshes[th.FULL]
    mb = th.mesh(*th.kuhn_mesh((10, 9, 8), (12, 0, 0)), th.wave_f, 0.3, normals=True,
                 cmap_seed=21, ntable=32)
    doms = []
    for m in (ma, mb):
        v, n, col, f = th.host_mesh(spray, m)
        doms.append((v, f, col, n))
    A, B = spray.RtContext(0), spray.RtContext(0)
    bounds = A.tet_isosurface_domains([0, 1], th.on_device([ma, mb]), bounds=True)
    for i, d in enumerate(doms):
        B.upload_domain(i, *d)
        assert bounds[i].tobytes() == np.concatenate([d[0].min(0), d[0].max(0)]).tobytes()
    for rt in (A, B):
        rt.domain_bounds(bounds)
        for i in range(2):
            rt.map_domain(i, i)
    allv = np.concatenate([doms[0][0], doms[1][0]])
    allf = np.concatenate([doms[0][1], doms[1][1] + len(doms[0][0])]).astype(np.uint32)
    org, d = rh.refit_rays(np.random.default_rng(5), allv, allf)
    rays = spray.make_rays(org, d)
    cam = oracle.camera_init([10.0, 5.0, 30.0], [10.0, 4.0, 3.0], [0, 1, 0], 60, 64, 64)
    eo, ed, pix, _ = oracle.eye_rays_ooc(cam, 64, 1, (0, 0, 64, 64))
    eye = spray.make_rays(eo, ed)
    ra = bh.scene_results(spray, A, rays, eye, pix)
    rb = bh.scene_results(spray, B, rays, eye, pix)
    # not vacuous: hits in both domains, mapped colours, both occlusion outcomes
    hits = np.frombuffer(ra["intersect_scene"], spray.HIT_DTYPE)
    assert set(np.unique(hits["domain"])) >= {-1, 0, 1}
    assert len(np.unique(hits["color"][hits["domain"] >= 0])) > 8
    occ = np.frombuffer(ra["occluded_scene_2"], np.uint8)
    assert 0 < occ.mean() < 1
    for k in ra:
        assert ra[k] == rb[k], k
    A.close()
    B.close()


def test_refit_recolor_replace_release(spray, oracle, meshes, restated):
    import torch
    v, n, col, f = restated[th.FULL]
    vu, fu = rh.mesh("grid12", oracle)
    c, B = spray.RtContext(0), spray.RtContext(0)
    c.upload_domain(2, vu, fu)                               # an uploaded slot is replaced
    c.tet_isosurface_domains([2], th.on_device([meshes[th.FULL]]))
    B.build_domains([2], [v], [f], [col], [n])
    assert export_all(c, 2) == export_all(B, 2)
    # a later refit
    v1 = rh.deform("sin", v)
    n1 = rh.vertex_normals(oracle, v1, f)
    for rt in (c, B):
        rt.refit_domains([2], [v1], [n1])
    assert export_all(c, 2) == export_all(B, 2)
    bh.check_queries(spray, oracle, c, 2, v1, f, col, n1, 73)
    # a recolour
    new = rh.vertex_colors(len(v))
    before = export_all(c, 2, KEPT)
    c.recolor_domains([2], [torch.from_numpy(new.view(np.int32)).cuda()])
    assert c.slot_export(2, c.SLOT_COLORS).tobytes() == new.tobytes()
    assert export_all(c, 2, KEPT) == before
    bh.check_queries(spray, oracle, c, 2, v1, f, new, n1, 74)
    # replaced by a smaller mesh, then by the empty surface, then released
    c.tet_isosurface_domains([2], [meshes[th.CUBE]])
    B.build_domains([2], [restated[th.CUBE][0]], [restated[th.CUBE][3]], [restated[th.CUBE][2]],
                    [restated[th.CUBE][1]])
    assert export_all(c, 2) == export_all(B, 2)
    c.tet_isosurface_domains([2], [meshes[th.EMPTY]])
    assert c.slot_info(2)["tris"] == 0
    c.release_domain(2)
    # and the context still extracts
    got = synced(c, c.tet_isosurface([meshes[th.CUBE]]))
    assert as_bytes(got[0]) == ref_bytes(restated[th.CUBE])
    c.close()
    B.close()


def test_failed_calls_change_nothing(spray, oracle, meshes, restated):
    va, fa = rh.mesh("grid12", oracle)
    c = spray.RtContext(0)
    c.upload_domain(0, va, fa)
    c.tet_isosurface_domains([1], [meshes[th.FULL]])
    before = (export_all(c, 0), export_all(c, 1))
    good = meshes[th.CUBE]
    src = meshes[th.PARTIAL]
    used = int(np.asarray(src["tets"])[1234, 2])

    def fails(bad, what, code=ERR_ARG):
        for ms in ([good, bad], th.on_device([good, bad])):
            for slots in ((0, 1), (1, 0)):   # the bad mesh aimed at either loaded slot
                with pytest.raises(spray.SprayRtError) as e:
                    c.tet_isosurface_domains(list(slots), ms)
                assert e.value.code == code and "mesh 1" in str(e.value) and what in str(e.value)
                assert (export_all(c, 0), export_all(c, 1)) == before
            with pytest.raises(spray.SprayRtError) as e:
                c.tet_isosurface(ms)
            assert e.value.code == code and "mesh 1" in str(e.value)

    def poked(key, index, value):
        a = np.array(src[key], copy=True)
        a[index] = value
        return dict(src, **{key: a})

    fails(poked("tets", (77, 1), len(src["points"])), "index")          # an index >= npoints
    fails(poked("values", used, np.nan), "sample")                      # a NaN value, referenced
    fails(poked("points", (used, 1), np.inf), "coordinate")
    fails(poked("normals", (used, 2), np.nan), "normal")
    mapped = th.mesh(src["points"], src["tets"], th.wave_f, 0.3, cmap_seed=31, ntable=8)
    cf = mapped["cfield"].copy()
    cf[used] = np.nan
    fails(dict(mapped, cfield=cf), "colour")                             # a NaN colour sample
    fails(dict(mapped, cmap=None), "table")
    fails(dict(src, iso=np.nan), "isovalue")

    # an unreferenced NaN point passes: nothing reads it
    p6 = np.vstack([src["points"], [[np.nan] * 3]]).astype(F32)
    extra = dict(src, points=p6, values=np.append(src["values"], F32(np.nan)),
                 normals=np.vstack([src["normals"], [[np.nan] * 3]]).astype(F32))
    ref = ref_bytes(restated[th.PARTIAL])
    for ms in ([extra], th.on_device([extra])):
        assert as_bytes(synced(c, c.tet_isosurface(ms))[0]) == ref
    # slots listed twice, and the good call goes through
    with pytest.raises(spray.SprayRtError) as e:
        c.tet_isosurface_domains([1, 1], [good, good])
    assert e.value.code == ERR_ARG and "slot 1" in str(e.value)
    assert (export_all(c, 0), export_all(c, 1)) == before
    c.tet_isosurface_domains([0], [good])
    assert c.slot_export(0, c.SLOT_FACES).tobytes() == restated[th.CUBE][3].tobytes()
    assert export_all(c, 1) == before[1]
    c.close()
