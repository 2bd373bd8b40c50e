// build_stages.hpp -- the device tree builder seen BETWEEN its stages (bvh_gpu.hip), and the same binary tree
// handed to the host's runs of stage 2 and stage 3.  Debug boundary only (include/pbrt_hip_debug.h): no production path sets an
// observer, and nothing here adds or changes a kernel.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "device_types.h"
#include "quad_nodes.hpp"
#include "reinsert_batch.hpp"

namespace pbrt_hip {

// A binary tree of n one-triangle leaves as BinaryTree (bvh_gpu.hip) holds it, copied to the host: interior nodes [0, n - 1), the
// root 0; a child word is an interior node or kLeafRef | leaf slot; in `boxes` (six floats per node: lo xyz, hi xyz) the leaf of
// slot k follows the interior nodes as node (n - 1) + k; order = leaf slot -> triangle.
struct StageTree {
  std::vector<uint32_t> child, parent_internal, parent_leaf, order;
  std::vector<float> boxes;
};

// What gpu_build_quads copies to the host, on the build's stream, when it is given one of these
struct GpuBuildStages {
  // after sah_build: the Morton keys as morton_kernel wrote them (before the sort) and the tree as built
  std::vector<uint32_t> morton_keys;
  StageTree built;
  // after the passes of reinsert, before ri_order_kernel (reinsert_ran = false: the tree was below the threshold, nothing else is set)
  bool reinsert_ran = false;
  std::vector<uint32_t> par, kid;  // reins::Tree's links
  std::vector<float> bx;           // ... and its boxes, six floats per node
  ReinsertStats reinsert;
  uint64_t visits = 0;             // nodes the searches looked at, summed over the passes (the undone one included)
  // after reinsert has returned (= built where it did not run)
  StageTree optimised;
  // collapse: the dynamic programme's tables (dp_ran = false: the greedy rule, no tables) as DpTables lays them out, rows of the
  // n - 1 interior nodes (F, G) and of the n leaf slots (Fl); then the quads, 16 words each
  bool dp_ran = false;
  std::vector<float> F, Fl, G;
  std::vector<uint32_t> quads;
  uint32_t n_quads = 0, stack_need = 0;
};

// ---- the host's runs of stages 2 and 3 on a tree given in BinaryTree's form (capi_scene.cpp checks the arguments) ----
// child[2 (n - 1)], boxes[6 (2 n - 1)] -> the link form reinsert_core.hpp works on, node for node as ri_links_kernel makes it.
// false (and *why): a child word out of range, a node that is not the child of exactly one node, or one the root does not reach.
bool link_tree_of_child_words(uint32_t n_tris, const uint32_t *child, const float *boxes, LinkTree *out, std::string *why);
// ... -> quad_nodes.cpp's collapse of that tree by rule `how` (kCollapseGreedy or kCollapseDp); a leaf child's slot is the tree's own
bool collapse_child_words(uint32_t n_tris, const uint32_t *child, const float *boxes, Collapse how, QuadNodes *out, std::string *why);

}  // namespace pbrt_hip
