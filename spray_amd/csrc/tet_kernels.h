// tet_kernels.h -- host-side launchers of the isosurface extraction from
// unstructured tetrahedral meshes (tet_kernels.hip): points, tets and samples
// in HBM to welded, indexed triangle meshes, batched over all meshes of a call.
//
// One thread per tetrahedron in blocks of tet::kTetBlock consecutive tets,
// then one thread per crossing-edge instance in blocks of as many sorted
// instances.  Nothing is handed between workgroups inside a launch: the count
// passes leave per-block sums, one workgroup per mesh turns them into block
// bases, the next launch reads them.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace spray_rt {

// What the host reads back per mesh: the sizes.
struct TetRec {
  uint64_t ninst, nfaces;  // crossing-edge instances and triangles (the first scan)
  uint64_t nverts;         // distinct crossing pairs (the second scan)
  uint64_t pad;
};

// One mesh of a call (device table).
struct alignas(16) TetJob {
  const float* points;     // [npoints][3]
  const uint32_t* tets;    // [ntets][4]
  const float* values;     // [npoints]
  const float* normals;    // [npoints][3]; nullptr: none, or not wanted
  const float* cfield;     // [npoints] colour field; nullptr: color
  const uint32_t* ctable;  // [ntable] device copy of the table
  uint32_t* word;          // [ntets] tet::tet_word per tet
  uint32_t* eblock;        // [nblocks] instances of each block, then its first instance
  uint32_t* fblock;        // [nblocks] the same for faces
  TetRec* rec;
  uint64_t npoints;
  uint32_t ntets, nblocks;
  float isovalue;
  uint32_t color;
  int32_t ntable;
  float clo, cscale;
  int32_t shift;  // tet::pair_key's
  uint32_t pad[2];
};
static_assert(sizeof(TetJob) % 16 == 0, "job table entries stay 16-B aligned");

// The instance scratch of one mesh, sized at the first host read (device table).
struct alignas(16) TetInst {
  uint64_t* keys;     // [ninst] pair keys in (tet, walk edge) order
  uint64_t* skeys;    // [ninst] sorted
  uint32_t* inst;     // [ninst] the instance index beside keys
  uint32_t* sinst;    // [ninst] ... beside skeys
  uint32_t* loc;      // [ninst] vertex id of a sorted instance within its block
  uint32_t* vid;      // [ninst] vertex id of every instance
  uint32_t* ublock;   // [niblocks] distinct keys of each block, then its first vertex
  uint32_t ninst, niblocks;
};
static_assert(sizeof(TetInst) % 16 == 0, "job table entries stay 16-B aligned");

// Where the last pass writes one mesh (device table); the capacities bound
// every store.
struct alignas(16) TetOut {
  float* verts;      // [nverts][3] or nullptr
  float* normals;    // [nverts][3] or nullptr
  uint32_t* colors;  // [nverts] or nullptr
  uint32_t* faces;   // [nfaces][3] or nullptr
  uint64_t cap_verts, cap_faces;
};
static_assert(sizeof(TetOut) % 16 == 0, "job table entries stay 16-B aligned");

// Count pass: a word per tet and per-block sums; what is wrong with a tet sets
// tet::kBad* bits in status[mesh].
hipError_t launch_tet_count(hipStream_t s, const TetJob* jobs, int njobs, uint32_t max_blocks,
                            uint32_t* status);
// Block sums to exclusive block bases, totals into rec (one workgroup per
// mesh): of eblock / fblock, or (unique) of ublock.
hipError_t launch_tet_scan(hipStream_t s, const TetJob* jobs, const TetInst* insts, int njobs,
                           bool unique);
// (key, instance) of every crossing walk edge at the tet's scanned offset.
hipError_t launch_tet_keys(hipStream_t s, const TetJob* jobs, const TetInst* insts, int njobs,
                           uint32_t max_blocks);
// rocPRIM segmented radix sort of (keys, inst) into (skeys, sinst): one
// segment per mesh, offsets[njobs + 1] in instances from the first mesh's
// arrays, key bits [0, end_bit).  tmp == nullptr: *tmp_bytes = the size.
hipError_t tet_sort(hipStream_t s, void* tmp, size_t* tmp_bytes, const uint64_t* keys,
                    uint64_t* skeys, const uint32_t* inst, uint32_t* sinst, uint32_t total,
                    int njobs, const uint32_t* offsets, unsigned end_bit);
// First-of-run flags of the sorted instances, scanned within each block.
hipError_t launch_tet_unique(hipStream_t s, const TetInst* insts, int njobs, uint32_t max_iblocks);
// Vertex ids to every instance; position, normal and colour of each distinct pair.
hipError_t launch_tet_verts(hipStream_t s, const TetJob* jobs, const TetInst* insts,
                            const TetOut* outs, int njobs, uint32_t max_iblocks);
// The triangles of every tet.
hipError_t launch_tet_faces(hipStream_t s, const TetJob* jobs, const TetInst* insts,
                            const TetOut* outs, int njobs, uint32_t max_blocks);

}  // namespace spray_rt
