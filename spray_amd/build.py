"""Builds libspray_rt.so (gfx950 kernels + C ABI + host scene layer) in-tree.

    python -m spray_amd.build          # or __graft_entry__.build()

The shared object lands in spray_amd/lib/ (git-ignored, shipped with the
tree to the GPU box).  Every translation unit is compiled with
-ffp-contract=off so fused multiply-adds happen only where the kernels write
fmaf() explicitly (bit parity with oracle/).
"""
from __future__ import annotations

import hashlib
import json
import os
import shutil
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(HERE, "csrc")
LIBDIR = os.path.join(HERE, "lib")
LIB = os.path.join(LIBDIR, "libspray_rt.so")
ARCH = os.environ.get("SPRAY_AMD_ARCH", "gfx950")

SOURCES = ["rt_kernels.hip", "ooc_kernels.hip", "frame_kernels.hip", "insitu_kernels.hip",
           "rt_api.cpp", "ooc.cpp", "frame.cpp", "insitu.cpp", "bvh_build.cpp", "scene_host.cpp",
           "footprint.cpp", "refit_kernels.hip", "refit.cpp", "build_kernels.hip",
           "build_device.cpp", "iso_kernels.hip", "isosurface.cpp", "tet_kernels.hip",
           "tet_isosurface.cpp", "cell_kernels.hip", "cell_isosurface.cpp", "surf_kernels.hip",
           "cell_surface.cpp", "clip_kernels.hip", "cell_clip.cpp", "stream_kernels.hip",
           "streamlines.cpp", "glyph_kernels.hip", "glyphs.cpp", "block_stream_kernels.hip",
           "block_streamlines.cpp"]
HEADERS = ["rt_common.h", "rt_device.h", "shade_device.h", "cam_device.h", "rt_kernels.h", "rt_ctx.h",
           "bvh_build.h", "scene_host.h", "insitu_kernels.h", "footprint.h", "refit_common.h",
           "refit_kernels.h", "build_common.h", "build_kernels.h", "iso_common.h",
           "iso_kernels.h", "job_arena.h", "block_scan.h", "color_common.h", "tet_common.h",
           "tet_kernels.h", "tet_pipeline.h", "cell_common.h", "cell_kernels.h",
           "surf_common.h", "surf_kernels.h", "clip_common.h", "clip_kernels.h",
           "stream_common.h", "stream_kernels.h", "glyph_common.h", "glyph_kernels.h",
           "stream_host.h", "block_stream_common.h", "block_stream_kernels.h"]
PUBLIC = [os.path.join(ROOT, "include", h) for h in ("spray_rt.h", "spray_scene.h")]


def hipcc():
    for c in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", shutil.which("hipcc")):
        if c and os.path.exists(c):
            return c
    raise RuntimeError("hipcc not found: the HIP engine cannot be built")


def _stale():
    if not os.path.exists(LIB):
        return True
    t = os.path.getmtime(LIB)
    deps = [os.path.join(CSRC, f) for f in SOURCES + HEADERS] + PUBLIC + [__file__]
    return any(os.path.getmtime(d) > t for d in deps)


def build(force=False, verbose=False, defines=(), out=None):
    """Builds the engine; `defines`/`out` produce diagnostic variants (never
    the shipped library)."""
    target = out or LIB
    if defines and out is None:
        # the shipped library's build id names its sources only; a variant
        # written over it would inherit that id (and the committed PMC
        # traffic of the clean build)
        raise ValueError("diagnostic defines need an explicit `out` path")
    if not force and not defines and out is None and not _stale():
        return LIB
    os.makedirs(os.path.dirname(target), exist_ok=True)
    tmp = target + ".tmp"
    flags = ["--offload-arch=" + ARCH, "-O3", "-std=c++17", "-fPIC",
             "-ffp-contract=off", "-fno-fast-math", "-Wall", "-Wno-unused-function",
             "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, *["-D" + d for d in defines]]
    cmd = [hipcc(), *flags, "-shared", *[os.path.join(CSRC, s) for s in SOURCES], "-ldl",
           "-o", tmp]
    # one translation unit per process (the kernels' TUs take most of the
    # time), then one link; the same flags and objects as the one-line form
    objdir = tmp + ".obj"
    os.makedirs(objdir, exist_ok=True)
    objs = [os.path.join(objdir, s + ".o") for s in SOURCES]

    def compile_one(k):
        c = [hipcc(), *flags, "-c", os.path.join(CSRC, SOURCES[k]), "-o", objs[k]]
        return subprocess.run(c, capture_output=True, text=True)

    if verbose:
        print(" ".join(cmd), file=sys.stderr)
    jobs = max(1, min(len(SOURCES), int(os.environ.get("MAX_JOBS", "0") or 0) or
                      (os.cpu_count() or 4)))
    with ThreadPoolExecutor(max_workers=min(jobs, 8)) as ex:
        res = list(ex.map(compile_one, range(len(SOURCES))))
    for s, r in zip(SOURCES, res):
        if r.returncode != 0:
            raise RuntimeError("hipcc failed on %s:\n%s%s" % (s, r.stdout, r.stderr))
    r = subprocess.run([hipcc(), *flags, "-shared", *objs, "-ldl", "-o", tmp],
                       capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError("hipcc link failed:\n" + r.stdout + r.stderr)
    shutil.rmtree(objdir, ignore_errors=True)
    os.replace(tmp, target)
    if target == LIB:
        # provenance of the shipped library: profiles/pmc_counters.json records
        # the id of the build it measured, bench.py checks it against this one
        with open(BUILD_INFO, "w") as fh:
            json.dump({"build_id": source_id(), "arch": ARCH,
                       "flags": [c for c in flags if not c.startswith("-I")]},
                      fh, indent=1)
    return target


BUILD_INFO = os.path.join(LIBDIR, "libspray_rt.build.json")


def source_id():
    """Hash of everything the shipped library is built from: the sources,
    the headers, the public headers and this file's compile line."""
    h = hashlib.sha256()
    h.update(ARCH.encode())
    for f in [os.path.join(CSRC, s) for s in SOURCES + HEADERS] + PUBLIC + [__file__]:
        h.update(os.path.basename(f).encode())
        with open(f, "rb") as fh:
            h.update(fh.read())
    return h.hexdigest()[:16]


def build_id():
    """The build id of the library in spray_amd/lib (None if it has none)."""
    try:
        with open(BUILD_INFO) as fh:
            return json.load(fh).get("build_id")
    except (OSError, ValueError):
        return None


TEST_SRC = os.path.join(ROOT, "tests", "cpp", "scene_adapter_test.cpp")
TEST_BIN = os.path.join(ROOT, "tests", "cpp", "_build", "scene_adapter_test")


def build_tests():
    """The C++ caller test of the SceneT drop-in (include/spray_scene.hpp):
    links the engine and the CPU oracle (test infrastructure)."""
    os.makedirs(os.path.dirname(TEST_BIN), exist_ok=True)
    cmd = ["g++", "-O2", "-std=c++17", "-fopenmp", "-ffp-contract=off", "-Wall",
           "-I" + os.path.join(ROOT, "include"),
           "-I" + os.path.join(ROOT, "oracle"), TEST_SRC, "-L" + LIBDIR, "-lspray_rt",
           "-L" + os.path.join(ROOT, "oracle", "_build"), "-loracle",
           "-Wl,-rpath,$ORIGIN/../../../spray_amd/lib:$ORIGIN/../../../oracle/_build",
           "-o", TEST_BIN]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError("scene adapter test build failed:\n" + r.stdout + r.stderr)
    return TEST_BIN


if __name__ == "__main__":
    print(build(force="--force" in sys.argv, verbose=True))
