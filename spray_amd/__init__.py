"""spray_amd -- MI355X-native BVH traversal + ray/triangle intersection engine
behind SpRay's scene intersect/occluded surface.

The engine is libspray_rt.so (hand-written gfx950 HIP kernels + C ABI, see
include/spray_rt.h and include/spray_scene.h); this package is its Python
binding.  There is no CPU fallback.
"""
from .engine import (HIT_DTYPE, INVALID_ID, RAY_DTYPE, RTC_ISECT_DTYPE, OocCache,
                     RtContext, Scene, SprayRtError, bvh_build_device_host, bvh_refit_host,
                     isosurface_host, isosurface_mapped_host, colormap_host, SLOT_COLORS,
                     SLOT_FACES, tet_isosurface_host, cell_isosurface_host, cell_split_host,
                     cell_surface_host, cell_clip_host, plane_values_host, camera_init, make_rays,
                     ooc_scene, streamlines_host, stream_tubes_host, tube_ring, block_streamlines_host,
                     block_stream_tubes_host, STREAM_FORWARD,
                     STREAM_BACKWARD, STREAM_BOTH, LINE_END_GRID, LINE_END_STEPS,
                     LINE_END_SPEED, LINE_END_SEED, glyphs_host, glyph_sphere, GLYPH_SPHERE,
                     GLYPH_ARROW)
from . import frame

__all__ = ["RtContext", "Scene", "OocCache", "ooc_scene", "SprayRtError", "camera_init",
           "make_rays", "bvh_refit_host", "bvh_build_device_host", "isosurface_host", "isosurface_mapped_host",
           "colormap_host", "tet_isosurface_host", "cell_isosurface_host", "cell_split_host", "cell_surface_host", "cell_clip_host", "plane_values_host", "streamlines_host", "stream_tubes_host", "tube_ring", "block_streamlines_host", "block_stream_tubes_host", "STREAM_FORWARD", "STREAM_BACKWARD", "STREAM_BOTH", "LINE_END_GRID", "LINE_END_STEPS", "LINE_END_SPEED", "LINE_END_SEED", "glyphs_host", "glyph_sphere", "GLYPH_SPHERE", "GLYPH_ARROW", "SLOT_COLORS", "SLOT_FACES", "RAY_DTYPE", "HIT_DTYPE", "RTC_ISECT_DTYPE", "INVALID_ID", "frame"]
