// quad_nodes.hpp -- the node arrays the kernels read, made on the host from a built binary tree: the child-pair records of the
// canonical walk and the 4-wide quantised nodes of the production walk (the record and the collapse's rules:
// quad_encode.hpp, shared with the device builder).  No HIP runtime call: the C boundary (capi_scene.cpp) uploads what comes out.
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include <hip/hip_vector_types.h>

#include "bvh_build.hpp"
#include "ref_bvh.hpp"
#include "reinsert_batch.hpp"

namespace pbrt_hip {

// "Children in parent" form of the binary tree for the kernels: one 64-byte record per INTERIOR
// node with the boxes and references of its two children.  ref = interior index
// (dense numbering of interior nodes in depth-first order) or kLeafRef | n_prims << 24 | first slot.
struct PairNodes {
  std::vector<uint4> q;  // 4 per interior node
  uint32_t root_ref = 0xffffffffu;
  float root_lo[3] = {0, 0, 0}, root_hi[3] = {0, 0, 0};
};
bool make_pair_nodes(const Bvh &b, PairNodes *out, std::string *why);

// 4-wide, QUANTISED form of the same tree for the production walk
struct QuadNodes {
  std::vector<uint4> q;     // 4 per node
  uint32_t stack_need = 0;  // most entries the walk can hold: max over root-to-leaf paths of sum(children - 1)
  std::vector<float> exact;  // diagnostics (tools/walk_sim.py): the children's boxes before quantisation, 24 floats per node
};
// which descendants become a quad node's children: both children of the binary node opened once, or quad_encode.hpp's rules
enum Collapse { kCollapsePlain = 0, kCollapseGreedy = 1, kCollapseDp = 2 };
// The rule for a tree of n_tris triangles: dp from quad::kDpCollapseMinTris on, greedy below; PBRT_HIP_COLLAPSE=dp|greedy|plain
// overrides (PBRT_HIP_GREEDY_COLLAPSE=0 = plain).  The device builder has no plain rule and keeps the size default there.
Collapse collapse_rule(size_t n_tris, bool has_plain = true);
// `b`: the binary tree over triangle references (the canonical tree through refs_of_bvh, or the optimised single-triangle tree of
// single_ref_tree + reinsert_optimize_batch); slot_of_ref[r] = slot of reference r's triangle in the leaf-ordered triangle records
// (null: r itself); split_leaves: a leaf of 2..4 triangles may become a quad node of single triangles, or open into the node above
void make_quad_nodes_as(const RefBvh &b, const uint32_t *slot_of_ref, bool split_leaves, Collapse how, QuadNodes *out);

// The production walk's 4-wide tree of a triangle soup, built on the host.  `tree` picks the binary tree it is collapsed from:
// kTreeCanonical = the canonical binned-SAH tree `canon` (the oracle's tree); kTreeReinsert = that tree with its
// leaves opened into single triangles and optimised by the DEVICE builder's parallel re-insertion pass run on the host
// (reinsert_batch.cpp: the same functions, reinsert_core.hpp).  Either way a leaf child's slot refers to the triangle records in
// `canon`'s leaf order.  (Round 3's host-only builders -- spatial splits, sequential re-insertion -- are records now:
// tools/experiments/r03_host_tree_builders/.)
enum ProductionTree : uint32_t { kTreeCanonical = 0, kTreeReinsert = 2 };  // (= PBRT_HIP_TREE_*)
ProductionTree production_tree_default();  // PBRT_HIP_TREE=reinsert, else the canonical tree
ReinsertBatchParams reinsert_batch_params();  // reins::StopRule's, shared with the device loop of bvh_gpu.hip (PBRT_HIP_REINSERT*)
void build_production_quads(const Bvh &canon, const float *P, const uint32_t *idx, uint32_t n_tris, ProductionTree tree,
                            bool split_leaves, QuadNodes *out, uint32_t *n_refs = nullptr);

}  // namespace pbrt_hip
