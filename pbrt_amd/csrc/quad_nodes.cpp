// quad_nodes.cpp -- see quad_nodes.hpp.  The host builder keeps what only it has (leaves of several triangles, split_leaves, the
// diagnostics array, the relayout aid) and takes every rule that decides a word of a record from quad_encode.hpp, as bvh_gpu.hip does.
#include "quad_nodes.hpp"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>

#include "build_stages.hpp"
#include "quad_encode.hpp"

namespace pbrt_hip {

namespace {
constexpr uint32_t kNoNode = 0xffffffffu;
inline uint32_t count_of(const BvhNode &n) { return n.count_axis & 0xffffu; }
}  // namespace

bool make_pair_nodes(const Bvh &b, PairNodes *out, std::string *why) {
  const size_t n = b.nodes.size();
  if (n == 0) return true;
  if (b.order.size() > (1u << 24)) { *why = "more than 2^24 triangles (leaf references hold a 24-bit slot)"; return false; }
  // Record numbering.  The memory system past L2 serves random requests in 128-byte lines at a rate
  // that does not depend on how many of the 128 bytes are used (tools/ubench/gather_wide.hip), so
  // the two 64-byte records of SIBLING interior nodes are placed in one line: fetching the near
  // child's record brings the far one along.  Sibling pairs start at even indices; groups follow
  // each other in depth-first order.  PBRT_HIP_NODE_LAYOUT=dfs restores plain depth-first numbering.
  std::vector<uint32_t> interior_index(n, 0);
  uint32_t n_int = 0;
  const char *layout = debug_knob("PBRT_HIP_NODE_LAYOUT");
  if (layout && std::string(layout) == "dfs") {
    for (size_t i = 0; i < n; i++)
      if (count_of(b.nodes[i]) == 0) interior_index[i] = n_int++;
  } else if (count_of(b.nodes[0]) == 0) {
    std::vector<uint32_t> todo = {0};
    interior_index[0] = 0;
    n_int = 2;  // the root has its line to itself
    while (!todo.empty()) {
      const uint32_t p = todo.back();
      todo.pop_back();
      const uint32_t c0 = p + 1, c1 = b.nodes[p].offset;
      const bool i0 = count_of(b.nodes[c0]) == 0, i1 = count_of(b.nodes[c1]) == 0;
      if (i0 && i1) {
        n_int = (n_int + 1u) & ~1u;
        interior_index[c0] = n_int;
        interior_index[c1] = n_int + 1;
        n_int += 2;
      } else if (i0) {
        interior_index[c0] = n_int++;
      } else if (i1) {
        interior_index[c1] = n_int++;
      }
      if (i1) todo.push_back(c1);
      if (i0) todo.push_back(c0);
    }
  }
  auto ref_of = [&](uint32_t i) -> uint32_t {
    const BvhNode &c = b.nodes[i];
    return count_of(c) ? quad::leaf_ref(count_of(c), c.offset) : interior_index[i];
  };
  auto as_u = quad::f32_bits;
  out->q.assign(4 * (size_t)n_int, make_uint4(0u, 0u, 0u, 0u));
  for (size_t i = 0; i < n; i++) {
    const BvhNode &p = b.nodes[i];
    if (count_of(p)) continue;
    const BvhNode &c0 = b.nodes[i + 1], &c1 = b.nodes[p.offset];
    uint4 *q = &out->q[4 * (size_t)interior_index[i]];
    q[0] = make_uint4(as_u(c0.lo[0]), as_u(c0.lo[1]), as_u(c0.lo[2]), as_u(c0.hi[0]));
    q[1] = make_uint4(as_u(c0.hi[1]), as_u(c0.hi[2]), as_u(c1.lo[0]), as_u(c1.lo[1]));
    q[2] = make_uint4(as_u(c1.lo[2]), as_u(c1.hi[0]), as_u(c1.hi[1]), as_u(c1.hi[2]));
    q[3] = make_uint4(ref_of((uint32_t)i + 1), ref_of(p.offset), p.count_axis >> 16, 0u);
  }
  out->root_ref = ref_of(0);
  for (int a = 0; a < 3; a++) { out->root_lo[a] = b.nodes[0].lo[a]; out->root_hi[a] = b.nodes[0].hi[a]; }
  return true;
}

namespace {

// A child of a quad node while it is being assembled: a node of the binary tree, or one triangle reference of an opened leaf
struct QuadChild {
  float lo[3], hi[3];
  uint32_t node, tri;  // (one of them is kNoNode)
};

// The collapse of one tree in three steps: dp_tables() bottom-up (the dp rule only), then per quad node, top-down,
// choose_children() / leaf_children() and emit().
struct QuadBuilder {
  struct Item { uint32_t node, quad, path; };  // binary node (a leaf: expanded into a node of its triangles), its quad, stack entries held above it
  const RefBvh &b;
  const uint32_t *slot_of_ref;
  const bool split_leaves;
  QuadNodes *out;
  std::vector<Item> todo;
  std::vector<float> F;  // F[(4 * n + (k - 1)) * 3 + (d - 1)]
  std::vector<float> G;  // work below n as a quad node of its own (interior nodes and splittable leaves)

  static size_t Fi(size_t n, uint32_t k, uint32_t d) { return (4 * n + (k - 1)) * 3 + (d - 1); }
  float operator()(uint32_t n, uint32_t k, uint32_t d) const { return F[Fi(n, k, d)]; }  // (the accessor quad_encode.hpp reads F through)
  uint32_t slot_of(uint32_t r) const { return slot_of_ref ? slot_of_ref[r] : r; }
  // a leaf of 2..4 triangles becomes a quad node of single triangles: their boxes are then tested in
  // the node step and each leaf pass tests exactly one triangle per parked lane
  bool splittable(const BvhNode &n) const { return split_leaves && count_of(n) >= 2 && count_of(n) <= 4; }

  QuadChild tri_child(uint32_t r) const {  // reference r, boxed by its own bounds
    QuadChild k{{0, 0, 0}, {0, 0, 0}, kNoNode, r};
    for (int a = 0; a < 3; a++) { k.lo[a] = b.ref_lo[3 * (size_t)r + a]; k.hi[a] = b.ref_hi[3 * (size_t)r + a]; }
    return k;
  }
  QuadChild node_child(uint32_t c) const {
    QuadChild k{{0, 0, 0}, {0, 0, 0}, c, kNoNode};
    for (int a = 0; a < 3; a++) { k.lo[a] = b.nodes[c].lo[a]; k.hi[a] = b.nodes[c].hi[a]; }
    return k;
  }
  int leaf_children(uint32_t leaf, QuadChild kids[4]) const {  // a leaf expanded: one child per triangle
    const BvhNode &n = b.nodes[leaf];
    for (uint32_t j = 0; j < count_of(n); j++) kids[j] = tri_child(n.offset + j);
    return (int)count_of(n);
  }

  // ---- step 1: F and G of every node, children before parents ----
  void dp_tables() {
    const size_t nn = b.nodes.size();
    F.assign(12 * nn, 0.f);
    G.assign(nn, 0.f);
    std::vector<uint32_t> parent(nn, kNoNode);
    for (size_t i = 0; i < nn; i++)
      if (count_of(b.nodes[i]) == 0) { parent[i + 1] = (uint32_t)i; parent[b.nodes[i].offset] = (uint32_t)i; }
    auto anc = [&](uint32_t n, uint32_t d) -> const BvhNode & {  // the ancestor at distance d (the root at most)
      while (d-- && parent[n] != kNoNode) n = parent[n];
      return b.nodes[n];
    };
    auto area_in = [](const float *lo, const float *hi, const BvhNode &q) { return quad::area_on_grid(lo, hi, q.lo, q.hi); };
    auto tris_in = [&](const BvhNode &leaf, const BvhNode &q) {  // the leaf's triangles as children of quad node q
      float w = 0.f;
      for (uint32_t j = 0; j < count_of(leaf); j++) { const QuadChild t = tri_child(leaf.offset + j); w += quad::kDpTriCost * area_in(t.lo, t.hi, q); }
      return w;
    };
    for (size_t i = nn; i-- > 0;) {  // children have larger indices than their parent (depth-first order)
      const BvhNode &n = b.nodes[i];
      const uint32_t cnt = count_of(n);
      const bool split = splittable(n);
      if (cnt == 0) G[i] = quad::dp_dist(*this, (uint32_t)i + 1, n.offset, 4u, 1u);
      else if (split) G[i] = tris_in(n, n);  // as a quad node of its own its triangles sit on ITS grid
      for (uint32_t d = 1; d <= 3; d++) {
        const BvhNode &q = anc((uint32_t)i, d);
        const float reach = area_in(n.lo, n.hi, q);
        // n presented as ONE child: a plain leaf has its triangles tested; else one step when reached, plus what lies below
        const float one = (cnt && !split) ? reach * quad::kDpTriCost * (float)cnt : reach + G[i];
        float f[4] = {one, one, one, one};
        if (cnt == 0) {
          quad::dp_interior(*this, (uint32_t)i + 1, n.offset, d, one, f);
        } else if (split) {  // opened: its triangles are direct children of the ancestor
          const float opened = std::min(one, tris_in(n, q));
          for (uint32_t k = cnt; k <= 4; k++) f[k - 1] = opened;
        }
        for (uint32_t k = 1; k <= 4; k++) F[Fi(i, k, d)] = f[k - 1];
      }
    }
    if (std::getenv("PBRT_HIP_REINSERT_VERBOSE"))
      std::fprintf(stderr, "collapse: expected work below the root G = %.4f root areas\n", G[0] / quad::box_area(b.nodes[0].lo, b.nodes[0].hi));
  }

  // ---- step 2: the children of the quad node made of binary interior node `node` ----
  int choose_children(uint32_t node, Collapse how, QuadChild kids[4]) const {
    const BvhNode &me = b.nodes[node];
    int nk = 0;
    if (how == kCollapseDp) {
      // follow the minimising choices: node c with k slots at distance d is opened or presented as one child
      struct Open { uint32_t c, k, d; };
      std::vector<Open> st;
      auto split = [&](uint32_t c, uint32_t k, uint32_t d) {  // the children of c share k slots at distance d
        const uint32_t l = c + 1, r = b.nodes[c].offset, kl = quad::dp_best_split(*this, l, r, k, d);
        st.push_back({r, k - kl, d});
        st.push_back({l, kl, d});
      };
      split(node, 4u, 1u);
      while (!st.empty()) {
        const Open o = st.back();
        st.pop_back();
        const BvhNode &n = b.nodes[o.c];
        if (count_of(n) == 0 && quad::dp_opens(*this, o.c, o.k, o.d)) {
          split(o.c, o.k, o.d + 1u);
        } else if (splittable(n) && o.k >= count_of(n) && (*this)(o.c, o.k, o.d) < (*this)(o.c, 1u, o.d)) {
          nk += leaf_children(o.c, kids + nk);  // opened: its triangles are direct children
        } else {
          kids[nk++] = node_child(o.c);
        }
      }
    } else if (how == kCollapseGreedy) {
      // start from the two children of the binary node and keep opening the child with the largest surface area (an
      // interior node into its two children, a small leaf into its triangles) while the result still fits four slots
      kids[nk++] = node_child(node + 1);
      kids[nk++] = node_child(me.offset);
      auto grow = [&](int k) {
        if (kids[k].node == kNoNode) return 0u;
        const BvhNode &n = b.nodes[kids[k].node];
        return count_of(n) == 0 ? 1u : (splittable(n) ? count_of(n) - 1u : 0u);
      };
      for (int best; (best = quad::greedy_pick(kids, nk, grow)) >= 0;) {
        const uint32_t c = kids[best].node;
        kids[best] = kids[--nk];
        if (count_of(b.nodes[c]) == 0) {
          kids[nk++] = node_child(c + 1);
          kids[nk++] = node_child(b.nodes[c].offset);
        } else {
          nk += leaf_children(c, kids + nk);
        }
      }
    } else {  // the plain collapse: both children opened once
      for (uint32_t c : {node + 1, me.offset}) {
        if (count_of(b.nodes[c]) == 0) { kids[nk++] = node_child(c + 1); kids[nk++] = node_child(b.nodes[c].offset); }
        else kids[nk++] = node_child(c);
      }
    }
    return nk;
  }

  // ---- step 3: the record of item `it` with children kids[0 .. nk); its interior children get their quads and are queued ----
  void emit(const Item &it, const QuadChild *kids, int nk) {
    const BvhNode &me = b.nodes[it.node];
    const uint32_t path = it.path + (uint32_t)(nk - 1);
    if (path > out->stack_need) out->stack_need = path;
    const quad::Grid grid = quad::quantise(me.lo, me.hi, kids, nk);
    uint32_t ref[4];
    for (int k = 0; k < 4; k++) {
      if (k >= nk) { ref[k] = kEmptyLeafRef; continue; }
      const BvhNode *n = kids[k].node != kNoNode ? &b.nodes[kids[k].node] : nullptr;
      if (!n) {
        ref[k] = quad::leaf_ref(1u, slot_of(kids[k].tri));
      } else if (count_of(*n) && !splittable(*n)) {
        ref[k] = quad::leaf_ref(count_of(*n), slot_of(n->offset));  // (a run of several references: consecutive slots)
      } else {  // an interior node, or a leaf that becomes a quad node of its triangles
        const uint32_t qi = (uint32_t)(out->q.size() / 4);
        ref[k] = quad::interior_ref(qi);
        out->q.resize(out->q.size() + 4, make_uint4(0, 0, 0, 0));
        // below child k the walk holds the entries of this path minus the ones already popped: bound by path
        todo.push_back({kids[k].node, qi, path});
      }
    }
    out->exact.resize(out->q.size() / 4 * 24, 0.f);
    for (int k = 0; k < 4; k++)
      for (int a = 0; a < 3; a++) {
        out->exact[(size_t)it.quad * 24 + k * 6 + a] = k < nk ? kids[k].lo[a] : std::numeric_limits<float>::infinity();
        out->exact[(size_t)it.quad * 24 + k * 6 + 3 + a] = k < nk ? kids[k].hi[a] : -std::numeric_limits<float>::infinity();
      }
    quad::pack_record(&out->q[4 * (size_t)it.quad], me.lo, grid, ref);
  }
};

}  // namespace

void make_quad_nodes_as(const RefBvh &b, const uint32_t *slot_of_ref, bool split_leaves, Collapse how, QuadNodes *out) {
  if (b.nodes.empty() || count_of(b.nodes[0]) != 0) return;  // no tree, or the root is a leaf
  QuadBuilder qb{b, slot_of_ref, split_leaves, out, {{0u, 0u, 0u}}, {}, {}};
  if (how == kCollapseDp) qb.dp_tables();
  out->q.assign(4, make_uint4(0, 0, 0, 0));
  while (!qb.todo.empty()) {
    const QuadBuilder::Item it = qb.todo.back();
    qb.todo.pop_back();
    QuadChild kids[4];
    const int nk = count_of(b.nodes[it.node]) ? qb.leaf_children(it.node, kids) : qb.choose_children(it.node, how, kids);
    qb.emit(it, kids, nk);
  }
}

// (build_stages.hpp) the collapse above over a tree in the device builder's form: flattened depth-first, reference r = leaf slot r
bool collapse_child_words(uint32_t n_tris, const uint32_t *child, const float *boxes, Collapse how, QuadNodes *out, std::string *why) {
  LinkTree lt;  // (checks every word, and that the words form one tree)
  if (!link_tree_of_child_words(n_tris, child, boxes, &lt, why)) return false;
  const uint32_t n_int = n_tris - 1u;
  RefBvh rb;
  rb.ref_tri.resize(n_tris);
  rb.ref_lo.resize(3 * (size_t)n_tris);
  rb.ref_hi.resize(3 * (size_t)n_tris);
  for (uint32_t r = 0; r < n_tris; r++) {
    rb.ref_tri[r] = r;
    for (int a = 0; a < 3; a++) { rb.ref_lo[3 * (size_t)r + a] = boxes[6 * (size_t)(n_int + r) + a]; rb.ref_hi[3 * (size_t)r + a] = boxes[6 * (size_t)(n_int + r) + 3 + a]; }
  }
  rb.nodes.reserve(2 * (size_t)n_tris);
  struct It { uint32_t node; int patch; };
  std::vector<It> st = {{0u, -1}};
  while (!st.empty()) {
    const It it = st.back();
    st.pop_back();
    const int me = (int)rb.nodes.size();
    if (it.patch >= 0) rb.nodes[it.patch].offset = (uint32_t)me;
    BvhNode b{};
    for (int a = 0; a < 3; a++) { b.lo[a] = boxes[6 * (size_t)it.node + a]; b.hi[a] = boxes[6 * (size_t)it.node + 3 + a]; }
    if (it.node >= n_int) { b.offset = it.node - n_int; b.count_axis = 1u; }
    rb.nodes.push_back(b);
    if (it.node < n_int) {
      st.push_back({lt.kid[2 * (size_t)it.node + 1], me});  // second child: patched when reached
      st.push_back({lt.kid[2 * (size_t)it.node], -1});      // first child: the next node
    }
  }
  make_quad_nodes_as(rb, nullptr, /*split_leaves=*/false, how, out);
  return true;
}

// A-B aid (PBRT_HIP_QUAD_LAYOUT=pre|pre_big behind the debug switch): renumber the quad nodes in depth-first PRE-order, so
// that a node and the first interior child visited after it share a 128-byte line (the collapse above keeps SIBLINGS
// together instead: a family is one or two lines).  pre: children in slot order; pre_big: the child with the largest box
// first.  The tree, and so every result, is unchanged.
static void relayout_quads(QuadNodes *q, bool big_first) {
  const size_t n = q->q.size() / 4;
  if (n < 2) return;
  auto area = [&](size_t node, int k) {
    const uint4 *w = &q->q[4 * node];
    auto byte = [](uint32_t v, int i) { return (float)((v >> (8 * i)) & 0xffu); };
    float cx, cy, cz;
    std::memcpy(&cx, &w[0].w, 4); std::memcpy(&cy, &w[2].z, 4); std::memcpy(&cz, &w[2].w, 4);
    const float dx = (byte(w[1].w, k) - byte(w[1].x, k)) * cx, dy = (byte(w[2].x, k) - byte(w[1].y, k)) * cy, dz = (byte(w[2].y, k) - byte(w[1].z, k)) * cz;
    return (dx * dy + dx * dz) + dy * dz;
  };
  std::vector<uint32_t> new_of(n, 0xffffffffu), order;
  order.reserve(n);
  std::vector<uint32_t> st = {0u};
  while (!st.empty()) {
    const uint32_t me = st.back();
    st.pop_back();
    new_of[me] = (uint32_t)order.size();
    order.push_back(me);
    const uint32_t ref[4] = {q->q[4 * (size_t)me + 3].x, q->q[4 * (size_t)me + 3].y, q->q[4 * (size_t)me + 3].z, q->q[4 * (size_t)me + 3].w};
    int ks[4], m = 0;
    for (int k = 0; k < 4; k++)
      if (!(ref[k] & kLeafRef)) ks[m++] = k;
    if (big_first) std::sort(ks, ks + m, [&](int a, int b) { return area(me, a) > area(me, b); });
    for (int i = m - 1; i >= 0; i--) st.push_back(quad::quad_of_ref(ref[ks[i]]));  // (the first of ks is popped next: it follows its parent)
  }
  std::vector<uint4> nq(q->q.size());
  std::vector<float> ne(q->exact.size());
  for (size_t i = 0; i < n; i++) {
    const size_t o = order[i];
    for (int w = 0; w < 4; w++) nq[4 * i + w] = q->q[4 * o + w];
    uint32_t *r = &nq[4 * i + 3].x;
    for (int k = 0; k < 4; k++)
      if (!(r[k] & kLeafRef)) r[k] = quad::interior_ref(new_of[quad::quad_of_ref(r[k])]);
    if (!ne.empty()) std::memcpy(&ne[24 * i], &q->exact[24 * o], 24 * sizeof(float));
  }
  q->q.swap(nq);
  q->exact.swap(ne);
}

Collapse collapse_rule(size_t n_tris, bool has_plain) {
  const Collapse by_size = n_tris >= quad::kDpCollapseMinTris ? kCollapseDp : kCollapseGreedy;
  const char *c = debug_knob("PBRT_HIP_COLLAPSE");
  const char *g = debug_knob("PBRT_HIP_GREEDY_COLLAPSE");
  if ((g && g[0] == '0') || (c && std::strcmp(c, "plain") == 0)) return has_plain ? kCollapsePlain : by_size;
  if (c && std::strcmp(c, "dp") == 0) return kCollapseDp;
  if (c && std::strcmp(c, "greedy") == 0) return kCollapseGreedy;
  return by_size;
}

// the tree the walk gets: collapsed by collapse_rule, renumbered if PBRT_HIP_QUAD_LAYOUT asks
static void make_quad_nodes(const RefBvh &b, const uint32_t *slot_of_ref, bool split_leaves, QuadNodes *out) {
  make_quad_nodes_as(b, slot_of_ref, split_leaves, collapse_rule(b.ref_tri.size()), out);
  if (const char *l = debug_knob("PBRT_HIP_QUAD_LAYOUT")) {
    if (std::strcmp(l, "pre") == 0) relayout_quads(out, false);
    else if (std::strcmp(l, "pre_big") == 0) relayout_quads(out, true);
  }
}

ReinsertBatchParams reinsert_batch_params() {
  ReinsertBatchParams p;
  if (const char *v = debug_knob("PBRT_HIP_REINSERT")) p.passes = std::atoi(v);
  if (const char *v = debug_knob("PBRT_HIP_REINSERT_MIN_TRIS")) p.stop.min_tris = (uint32_t)std::max(8, std::atoi(v));
  if (const char *v = debug_knob("PBRT_HIP_REINSERT_MU")) p.mu = (uint32_t)std::max(1, std::atoi(v));
  if (const char *v = debug_knob("PBRT_HIP_REINSERT_VISITS")) p.search.max_visits = (uint32_t)std::max(1, std::atoi(v));
  if (const char *v = debug_knob("PBRT_HIP_REINSERT_MIN_REL")) p.search.min_rel = (float)std::atof(v);
  if (const char *v = debug_knob("PBRT_HIP_REINSERT_QK")) p.search.qk = (float)std::atof(v);
  if (const char *v = debug_knob("PBRT_HIP_REINSERT_QW")) p.search.qw = (float)std::atof(v);
  return p;
}
ProductionTree production_tree_default() {
  const char *v = debug_knob("PBRT_HIP_TREE");
  if (v && std::strcmp(v, "reinsert") == 0) return kTreeReinsert;
  return kTreeCanonical;
}
void build_production_quads(const Bvh &canon, const float *P, const uint32_t *idx, uint32_t n_tris, ProductionTree tree,
                            bool split_leaves, QuadNodes *out, uint32_t *n_refs) {
  RefBvh rb;
  if (tree == kTreeReinsert && n_tris >= 2) {
    single_ref_tree(canon, P, idx, &rb);
    const ReinsertBatchParams rp = reinsert_batch_params();
    if (n_tris >= rp.stop.min_tris) reinsert_optimize_batch(&rb, rp);  // (smaller trees stay as built, as on the device)
    if (std::getenv("PBRT_HIP_REINSERT_VERBOSE")) {
      LinkTree lt;
      link_tree_of(rb, &lt);
      std::fprintf(stderr, "tree %u: summed interior half-area %.6g, depth %u\n", (unsigned)tree, lt.cost(), rb.depth);
    }
    std::vector<uint32_t> slot_of_tri(n_tris), slot_of_ref(rb.ref_tri.size());
    for (uint32_t s = 0; s < n_tris; s++) slot_of_tri[canon.order[s]] = s;
    for (size_t r = 0; r < rb.ref_tri.size(); r++) slot_of_ref[r] = slot_of_tri[rb.ref_tri[r]];
    make_quad_nodes(rb, slot_of_ref.data(), true, out);
  } else {
    refs_of_bvh(canon, P, idx, &rb);
    make_quad_nodes(rb, nullptr, split_leaves, out);
  }
  if (n_refs) *n_refs = (uint32_t)rb.ref_tri.size();
}

}  // namespace pbrt_hip
