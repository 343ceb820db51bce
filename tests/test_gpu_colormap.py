"""Colour maps on the GPU (spray_rt_isosurface_mapped,
spray_rt_domains_isosurface_mapped, spray_rt_colormap_apply,
spray_rt_domains_recolor).

References, each bit for bit: the host restatements
(spray_rt_isosurface_mapped_host, spray_rt_colormap_host) for the extracted
arrays and colours, spray_rt_isosurface for the geometry, a build_domains of
the restated arrays in a second context for the slot images, an upload of the
same meshes for the scene launch, the oracle's brute force for queries.
"""
import numpy as np
import pytest

import build_helpers as bh
import color_helpers as ch
import refit_helpers as rh

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_LIMIT = -1, -5
CELL, PLAIN, SPHERE, TORUS, BLOCKS, WAVELET, EMPTY = range(7)
WHAT = bh.WHAT + ("COLORS", "FACES")
KEPT = tuple(w for w in WHAT if w != "COLORS")


@pytest.fixture(scope="module")
def spray():
    import torch  # noqa: F401  (one HIP runtime in the process)
    import spray_amd
    return spray_amd


@pytest.fixture(scope="module")
def grids():
    return ch.gpu_grids()


@pytest.fixture(scope="module")
def restated(spray, grids):
    """(verts, normals, colors, faces) of every grid from the host restatement."""
    return [ch.host_mesh(spray, g) for g in grids]


def slot_colors(g, col):
    """The colour array a slot of grid g carries: none without a field or a colour."""
    return col if g.get("cfield") is not None or g.get("color") is not None else None


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


def test_batch_shapes(grids, restated):
    """The grids reach the paths they are there for."""
    assert [g.get("cfield") is not None for g in grids] == [True, False, False, True, True, True, True]
    assert grids[PLAIN].get("color") is None and grids[SPHERE]["color"] is not None
    assert grids[CELL]["values"].shape == (2, 2, 2) and len(restated[CELL][2]) > 0
    assert grids[BLOCKS]["values"].size > 4 * 256
    assert grids[WAVELET]["values"].size > 512 * 256
    assert len(restated[EMPTY][0]) == 0
    for k in (CELL, TORUS, WAVELET):   # several bins, and both ends of a clamped range
        assert len(np.unique(restated[k][2])) > 3
    tab = grids[TORUS]["cmap"][0]
    assert {int(tab[0]), int(tab[-1])} <= set(restated[TORUS][2].tolist())
    assert (restated[SPHERE][2] == grids[SPHERE]["color"]).all()
    assert (restated[PLAIN][2] == 0).all() and len(restated[PLAIN][2]) > 0


@pytest.mark.parametrize("device", [True, False], ids=["tensors", "numpy"])
def test_kernels_equal_the_host_restatement(spray, grids, restated, device):
    c = spray.RtContext(0)
    gs = ch.on_device(grids) if device else grids
    got = [as_bytes(m) for m in synced(c, c.isosurface_mapped(gs))]
    plain = [as_bytes(m) for m in synced(c, c.isosurface(gs))]
    for k, ref in enumerate(restated):
        assert got[k] == ref_bytes(ref), k
        assert (got[k][0], got[k][1], got[k][3]) == plain[k], k
    # the same batch in reversed order, without normals: the same bytes per grid
    rev = [as_bytes(m) for m in synced(c, c.isosurface_mapped(gs[::-1], normals=False))][::-1]
    for k in range(len(grids)):
        assert rev[k] == (got[k][0], None, got[k][2], got[k][3]), k
    c.close()


def test_colors_only_form(spray, grids, restated):
    c = spray.RtContext(0)
    gs = ch.on_device(grids)
    got = synced(c, c.isosurface_mapped(gs, colors_only=True))
    for k, (v, n, col, f) in enumerate(got):
        assert v is None and n is None and f is None
        assert col.cpu().numpy().tobytes() == restated[k][2].tobytes(), k
    nv = len(restated[TORUS][0])
    with pytest.raises(spray.SprayRtError) as e:
        c.isosurface_mapped([gs[SPHERE], gs[TORUS]], capacity=(nv - 1, 0), colors_only=True)
    assert e.value.code == ERR_LIMIT and "grid 1" in str(e.value)
    assert e.value.counts == [(len(restated[k][0]), len(restated[k][3])) for k in (SPHERE, TORUS)]
    c.sync()
    for bufs in e.value.buffers:   # zeroed before the call: untouched
        assert all(int(b.abs().max()) == 0 for b in bufs)
    # the exact vertex capacity fits, whatever the faces'
    got = synced(c, c.isosurface_mapped([gs[TORUS]], capacity=(nv, 0), colors_only=True))
    assert got[0][2].cpu().numpy().tobytes() == restated[TORUS][2].tobytes()
    # the full form into short buffers: nothing written either
    with pytest.raises(spray.SprayRtError) as e:
        c.isosurface_mapped([gs[TORUS]], capacity=(nv, len(restated[TORUS][3]) - 1))
    assert e.value.code == ERR_LIMIT
    c.sync()
    for bufs in e.value.buffers:
        assert all(int(b.abs().max()) == 0 for b in bufs)
    c.close()


def test_slot_images_equal_a_build_of_the_restated_arrays(spray, grids, restated):
    n = len(grids)
    c, B = spray.RtContext(0), spray.RtContext(0)
    bounds = c.isosurface_domains_mapped(list(range(n)), ch.on_device(grids), bounds=True)
    cols = [slot_colors(g, r[2]) for g, r in zip(grids, restated)]
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
    # numpy fields, other slots, no normals
    c.isosurface_domains_mapped([9, 8], [grids[TORUS], grids[CELL]], normals=False)
    B.build_domains([9, 8], [restated[TORUS][0], restated[CELL][0]],
                    [restated[TORUS][3], restated[CELL][3]],
                    [restated[TORUS][2], restated[CELL][2]])
    for k in (9, 8):
        assert export_all(c, k) == export_all(B, k), k
    c.close()
    B.close()


def scene_hits(spray, rt, bounds, rays):
    rt.domain_bounds(bounds)
    for i in range(len(bounds)):
        rt.map_domain(i, i)
    return rt.intersect_scene(rays.copy())


def test_scene_hits_equal_uploaded_slots(spray, grids):
    ga = dict(grids[TORUS], origin=(9.0, -4.0, -5.0))
    gb = ch.mapped(dict(grids[SPHERE]), 77, 32)
    doms = []
    for g in (ga, gb):
        v, n, col, f = ch.host_mesh(spray, g)
        doms.append((v, f, col, n))
    A, B, K = spray.RtContext(0), spray.RtContext(0), spray.RtContext(0)
    bounds = A.isosurface_domains_mapped([0, 1], ch.on_device([ga, gb]), bounds=True)
    for i, d in enumerate(doms):
        B.upload_domain(i, *d)
    # the parent's path: one constant colour per grid
    const = [dict(g, cfield=None, cmap=None, color=0x00102030) for g in (ga, gb)]
    K.isosurface_domains([0, 1], const)
    allv = np.concatenate([doms[0][0], doms[1][0]])
    allf = np.concatenate([doms[0][1], doms[1][1] + len(doms[0][0])]).astype(np.uint32)
    org, d = rh.refit_rays(np.random.default_rng(5), allv, allf)
    rays = spray.make_rays(org, d)
    ha, hb, hk = (scene_hits(spray, rt, bounds, rays) for rt in (A, B, K))
    assert set(np.unique(ha["domain"])) >= {-1, 0, 1}
    assert ha.tobytes() == hb.tobytes()
    hit = ha["domain"] >= 0
    assert len(np.unique(ha["color"][hit])) > 8
    for name in ha.dtype.names:
        same = ha[name].tobytes() == hk[name].tobytes()
        assert same == (name != "color"), name
    for rt in (A, B, K):
        rt.close()


def test_recolor(spray, oracle, grids, restated):
    import torch
    v, n, col, f = restated[TORUS]
    vs, ns, cs, fs = restated[SPHERE]
    c = spray.RtContext(0)
    c.build_domains([2, 5], [v, vs], [f, fs], [col, cs], [n, ns])
    before = {k: export_all(c, k, KEPT) for k in (2, 5)}
    new = {2: rh.vertex_colors(len(v)), 5: rh.vertex_colors(len(vs))[::-1].copy()}
    # from device pointers, both slots in one call
    c.recolor_domains([5, 2], [torch.from_numpy(new[k].view(np.int32)).cuda() for k in (5, 2)])
    for k in (2, 5):
        assert c.slot_export(k, c.SLOT_COLORS).tobytes() == new[k].tobytes()
        assert export_all(c, k, KEPT) == before[k]
    bh.check_queries(spray, oracle, c, 2, v, f, new[2], n, 61)
    B = spray.RtContext(0)
    B.build_domains([2, 5], [v, vs], [f, fs], [new[2], new[5]], [n, ns])
    for k in (2, 5):
        assert export_all(c, k) == export_all(B, k)
    # from a host pointer
    newer = (new[2] ^ np.uint32(0x00FF00FF)).astype(np.uint32)
    c.recolor_domains([2], [newer])
    assert c.slot_export(2, c.SLOT_COLORS).tobytes() == newer.tobytes()
    assert export_all(c, 2, KEPT) == before[2]
    assert c.slot_export(5, c.SLOT_COLORS).tobytes() == new[5].tobytes()
    bh.check_queries(spray, oracle, c, 2, v, f, newer, n, 62)
    # a later refit keeps the new colours
    v1 = rh.deform("sin", v)
    n1 = rh.vertex_normals(oracle, v1, f)
    c.refit_domains([2], [v1], [n1])
    assert c.slot_export(2, c.SLOT_COLORS).tobytes() == newer.tobytes()
    bh.check_queries(spray, oracle, c, 2, v1, f, newer, n1, 63)
    B.close()
    c.close()


def test_isosurface_recolor_equals_a_fresh_extraction(spray, grids):
    pick = [TORUS, WAVELET, SPHERE, EMPTY]
    old = ch.on_device([grids[k] for k in pick])
    fresh = []
    for k, g in zip(pick, old):   # another table and range, and another field for one
        g = dict(g)
        if g.get("cfield") is not None:
            tab, lo, hi = g["cmap"]
            g["cmap"] = (ch.table(len(tab) // 2 + 3, 200 + k), lo - 0.1, hi + 0.3)
        fresh.append(g)
    fresh[0]["cfield"] = (fresh[0]["cfield"] * 0.5 + 0.1).contiguous()
    fresh[2] = dict(fresh[2], color=0x00445566)      # a constant colour changes too
    slots = [4, 1, 7, 2]
    c, B = spray.RtContext(0), spray.RtContext(0)
    c.isosurface_domains_mapped(slots, old)
    B.isosurface_domains_mapped(slots, fresh)
    assert export_all(c, 4)["COLORS"] != export_all(B, 4)["COLORS"]
    cols = [m[2] for m in c.isosurface_mapped(fresh, colors_only=True)]
    c.recolor_domains(slots, cols)
    for s in slots:
        assert export_all(c, s) == export_all(B, s), s
    c.close()
    B.close()


@pytest.fixture(scope="module")
def apply_case():
    rng = np.random.default_rng(3)
    x = rng.uniform(-1.5, 2.5, 1100).astype(np.float32)
    x[:6] = [-1.0, 2.0, -3e38, 3e38, 0.0, -0.0]
    return x, (ch.table(100, 5), -1.0, 2.0)


@pytest.mark.parametrize("n", [0, 1, 3, 4, 5, 63, 64, 65, 1027])
def test_colormap_apply_equals_the_host(spray, apply_case, n):
    import torch
    x, cmap = apply_case
    c = spray.RtContext(0)
    ref = spray.colormap_host(x[:n + 1], *cmap)
    d = torch.from_numpy(x).cuda()
    assert c.colormap_apply(d[:n], cmap).cpu().numpy().view(np.uint32).tobytes() == ref[:n].tobytes()
    assert c.colormap_apply(x[:n], cmap).cpu().numpy().view(np.uint32).tobytes() == ref[:n].tobytes()
    # both pointers one element past a 16-B boundary, then only one of them
    for so, oo in ((1, 1), (1, 0), (0, 3), (2, 2)):
        out = torch.full((n + 8,), 0x55, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()   # filled before the context's stream writes it
        c.colormap_apply(d[so:so + n], cmap, out=out[oo:oo + n])
        got = out.cpu().numpy()
        assert got[oo:oo + n].view(np.uint32).tobytes() == \
            spray.colormap_host(x[so:so + n], *cmap).tobytes(), (so, oo)
        assert (got[:oo] == 0x55).all() and (got[oo + n:] == 0x55).all()   # nothing beside it
    c.close()


def test_colormap_apply_errors(spray, apply_case):
    import torch
    x, cmap = apply_case
    c = spray.RtContext(0)
    bad = x[:70].copy()
    bad[37] = np.nan
    for arg in (bad, torch.from_numpy(bad).cuda()):
        with pytest.raises(spray.SprayRtError) as e:
            c.colormap_apply(arg, cmap)
        assert e.value.code == ERR_ARG and "non-finite" in str(e.value)
    for m in ((cmap[0], 2.0, 2.0), (np.zeros(0, np.uint32), 0.0, 1.0), (cmap[0], -3e38, 3e38)):
        with pytest.raises(spray.SprayRtError) as e:
            c.colormap_apply(x[:8], m)
        assert e.value.code == ERR_ARG
    # the context still works
    assert c.colormap_apply(x[:9], cmap).cpu().numpy().view(np.uint32).tobytes() == \
        spray.colormap_host(x[:9], *cmap).tobytes()
    c.close()


def test_failed_calls_change_nothing(spray, oracle, grids, restated):
    import torch
    va, fa = rh.mesh("grid12", oracle)
    na = rh.vertex_normals(oracle, va, fa)
    c = spray.RtContext(0)
    c.upload_domain(0, va, fa, None, na)                       # a slot without colours
    c.isosurface_domains_mapped([1], [grids[TORUS]])
    before = (export_all(c, 0), export_all(c, 1))
    good = grids[SPHERE]

    def unchanged():
        assert (export_all(c, 0), export_all(c, 1)) == before

    def mapped_fails(gs, slots=(0, 1), names="grid 1"):
        with pytest.raises(spray.SprayRtError) as e:
            c.isosurface_domains_mapped(list(slots), gs)
        assert e.value.code == ERR_ARG and names in str(e.value)
        unchanged()
        with pytest.raises(spray.SprayRtError) as e:
            c.isosurface_mapped(gs)
        assert e.value.code == ERR_ARG and names in str(e.value)

    tor = grids[TORUS]
    nan = tor["cfield"].copy()
    nan[9, 3, 11] = np.inf
    for tgt in (0, 1):   # the bad grid aimed at either loaded slot, second in the call
        mapped_fails([good, dict(tor, cfield=nan)], (1 - tgt, tgt))
        mapped_fails(ch.on_device([good, dict(tor, cfield=nan)]), (1 - tgt, tgt))
    tab = tor["cmap"][0]
    mapped_fails([good, dict(tor, cmap=None)])                               # no table
    mapped_fails([good, dict(tor, cmap=(np.zeros(4097, np.uint32), 0.0, 1.0))])
    mapped_fails([good, dict(tor, cmap=(tab, 1.0, 1.0))])
    mapped_fails([good, dict(tor, cmap=(tab, np.nan, 1.0))])
    mapped_fails([good, dict(tor, cmap=(tab, -3e38, 3e38))])                 # scale 0
    mapped_fails([dict(tor, cmap=(tab, 0.0, 1e-45)), good], names="grid 0")  # scale inf

    def recolor_fails(slots, cols, names):
        with pytest.raises(spray.SprayRtError) as e:
            c.recolor_domains(slots, cols)
        assert e.value.code == ERR_ARG and names in str(e.value)
        unchanged()

    nv = len(restated[TORUS][0])
    ok = rh.vertex_colors(nv)
    dev = torch.from_numpy(ok.view(np.int32)).cuda()
    for arr in (ok, dev):
        recolor_fails([1, 0], [arr, rh.vertex_colors(len(va))], "slot 0")   # no colours
        recolor_fails([1, 6], [arr, arr], "slot 6")                         # not loaded
        recolor_fails([1, 1], [arr, arr], "slot 1")                         # listed twice
        recolor_fails([1], [arr[:nv - 1]], "slot 1")                        # wrong nverts
    recolor_fails([1], [None], "slot 1")
    # and the good call goes through
    c.recolor_domains([1], [dev])
    assert c.slot_export(1, c.SLOT_COLORS).tobytes() == ok.tobytes()
    assert export_all(c, 1, KEPT) == {k: before[1][k] for k in KEPT}
    assert export_all(c, 0) == before[0]
    c.close()
