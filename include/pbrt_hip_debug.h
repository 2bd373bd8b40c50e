/*
 * pbrt_hip_debug.h -- test and measurement hooks of libpbrt_hip.so.  NOT part of the boundary a host binds (that is
 * pbrt_hip.h: SURVEY.md 8(b)'s calls, the multi-GPU entry points, the loader, image I/O, the Film helpers): these entry
 * points exist so that tests/ can check the trees the builders make, tools/ can cost them without a GPU, and the parser's
 * conformance tests can look at its state.  They may change between versions.  Each cites what it stands in for, as there.
 */
#ifndef PBRT_HIP_DEBUG_H
#define PBRT_HIP_DEBUG_H
#include "pbrt_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

/* ---- the accelerator as built (the reference names one, core/api.rs:237 "bvh", and builds none) ---- */
/* the canonical tree behind the counter flags: *ready = it exists (always for a host-built scene; for a device-built one
 * after the first call that counted), *build_ms = the host builder's time for it */
int pbrt_hip_scene_canonical_info(const pbrt_hip_scene *scene, uint32_t *ready, double *build_ms);
/* the objective of the device build's tree optimisation (pbrt_hip_scene_optimize_info: passes, moves, time): the summed half surface
 * area of the interior nodes of the binary tree before the first pass and after the last one kept; *undone = 1 when a pass raised
 * it, was undone and ended the passes (pbrt_amd/csrc/reinsert_core.hpp).  Zeros for a host-built scene.  Any pointer may be NULL. */
int pbrt_hip_scene_optimize_cost(const pbrt_hip_scene *scene, double *before, double *after, uint32_t *undone);
/* the production walk's tree as it sits in HBM: quads = 16 words per node (cap_nodes of them), order = leaf slot ->
 * triangle id (n_tris words); either may be NULL */
int pbrt_hip_scene_export_quads(const pbrt_hip_scene *scene, uint32_t *quads, uint32_t cap_nodes, uint32_t *n_quads,
                                uint32_t *order);
/* the canonical binary tree, host copy: 8 words per node; order maps leaf slot -> triangle id */
int pbrt_hip_scene_export_bvh(const pbrt_hip_scene *scene, uint32_t *nodes /* 8 words each */, uint32_t *order);
/* the production walk's own structure: number of 64-byte quantised 4-wide nodes, and the most stack entries a
 * walk can hold (see pbrt_hip_render_stack_plan for where they live) */
int pbrt_hip_scene_walk_info(const pbrt_hip_scene *scene, uint32_t *quad_nodes, uint32_t *stack_need);
/* How the render kernel is launched for a tree with that stack bound (pure function, no device touched): LDS rows of
 * 64 x 4 bytes per wave, one-wave workgroups a CU holds at once with them (the grid is this x the CU count), and the
 * entries per lane kept in an HBM overflow area (non-zero = the overflow variant of the kernel). */
int pbrt_hip_render_stack_plan(uint32_t stack_need, uint32_t *lds_rows, uint32_t *waves_per_cu, uint32_t *overflow_entries);
/* The same for the default path's launch (no counters, box filter radius 0.5, samplers 0 / 1, no MIS, textures, glass, map or shading
 * normals), whose overflow variant keeps three 1 KB path-state records per wave in LDS behind a shorter stack: the stack's rows, the
 * bytes of the records behind them (0 = the records are in HBM: every tree that keeps its whole stack in LDS), the workgroups per CU
 * and the overflow entries per lane.  Every other launch is pbrt_hip_render_stack_plan's. */
int pbrt_hip_render_stack_layout(uint32_t stack_need, uint32_t *stack_rows, uint32_t *record_bytes, uint32_t *waves_per_cu,
                                 uint32_t *overflow_entries);
/* the librccl the in-library multi-GPU path uses (pbrt_hip_multi_*: loaded on first use by dlopen): its file name -- it must be the one
 * that belongs to the HIP runtime of the process (beside the loaded libamdhip64), whichever host loaded that.  No device is touched. */
int pbrt_hip_rccl_library(char *path, size_t cap);
/* host-only variant for CPU-side tests of the builder: no device is touched */
int pbrt_hip_bvh_build_host(const float *P, uint32_t n_verts, const uint32_t *idx, uint32_t n_tris,
                            uint32_t *nodes /* 8*(2*n_tris) words cap */, uint32_t *order, uint32_t *n_nodes,
                            uint32_t *depth);

/* host-only: the production walk's quantised 4-wide tree from a triangle soup, for CPU-side
 * tests of its invariants.  quads: 16 words per node (cap_nodes nodes of room); split_leaves as the library default. */
int pbrt_hip_quad_build_host(const float *P, uint32_t n_verts, const uint32_t *idx, uint32_t n_tris, int split_leaves,
                             uint32_t *quads, uint32_t cap_nodes, uint32_t *n_quads, uint32_t *stack_need);
/* The same with the binary tree the 4-wide nodes are collapsed from chosen explicitly -- PBRT_HIP_TREE_SAH: the canonical
 * binned-SAH tree of DESIGN.md 3.3; PBRT_HIP_TREE_REINSERT: that tree with its leaves opened into single triangles and optimised
 * by the device builder's parallel re-insertion pass RUN ON THE HOST (the same functions, pbrt_amd/csrc/reinsert_core.hpp: what
 * lets the CPU tests walk the trees that pass makes; PBRT_HIP_SCENE_OPTIMIZED_TREE's tree) -- and more outputs, each of which may
 * be NULL: order = leaf slot -> triangle id (n_tris words; what a leaf child's slot refers to), root_box = lo xyz, hi xyz, n_refs
 * = references in the tree (n_tris), exact_boxes = the children's boxes before quantisation (24 floats per node of `quads`: lo
 * xyz, hi xyz of child 0..3; diagnostics).  (Round 3's PBRT_HIP_TREE_SBVH = 1, a spatial-split builder measured negative on
 * BASELINE's meshes, is no longer in the library: tools/experiments/r03_host_tree_builders/.) */
#define PBRT_HIP_TREE_SAH 0u
#define PBRT_HIP_TREE_REINSERT 2u
#define PBRT_HIP_TREE_DEFAULT 0xffffffffu
int pbrt_hip_quad_build_host_ex(const float *P, uint32_t n_verts, const uint32_t *idx, uint32_t n_tris, int split_leaves,
                                uint32_t tree, uint32_t *quads, uint32_t cap_nodes, uint32_t *n_quads, uint32_t *stack_need,
                                uint32_t *order, float *root_box, uint32_t *n_refs, float *exact_boxes);

/* ---- the device tree builder between its stages (pbrt_amd/csrc/bvh_gpu.hip) ---- */
/* A binary tree of n one-triangle leaves in the device builder's form: interior nodes [0, n - 1), the root 0; child = 2 (n - 1) words, an
 * interior node or 0x80000000 | leaf slot; parent_internal (n - 1 words; the root's: 0xffffffff) and parent_leaf (n words, by slot); boxes =
 * six floats (lo xyz, hi xyz) per node, the leaf of slot k following the interior nodes as node (n - 1) + k; order = leaf slot -> triangle.
 * The LINK form re-insertion works on (pbrt_amd/csrc/reinsert_core.hpp): nodes [0, 2 n - 1) numbered as in `boxes`, par (2 n - 1 words; the
 * root's: 0xffffffff), kid (2 (n - 1) words), boxes as above.
 * The arrays of HOST memory the device hook fills, each of which may be NULL, and the scalars it sets: */
typedef struct pbrt_hip_build_stages {
  uint32_t *morton_keys;  /* n: as morton_kernel wrote them, before the sort */
  uint32_t *built_child, *built_parent_internal, *built_parent_leaf;  /* the tree after stage 1 (sah_build) */
  float *built_boxes;
  uint32_t *built_order;
  uint32_t *links_par, *links_kid;  /* the link form after the passes of stage 2, before the child order (written when reinsert_ran) */
  float *links_boxes;
  uint32_t *opt_child, *opt_parent_internal, *opt_parent_leaf;  /* the tree stage 3 collapses (= built where stage 2 did not run) */
  float *opt_boxes;
  uint32_t *opt_order;
  float *dp_F, *dp_Fl, *dp_G;  /* written when dp_ran: F[(4 node + k - 1) 3 + d - 1] of the n - 1 interior nodes, Fl[3 slot + d - 1], G[node] */
  uint32_t *quads;             /* 16 words per quad node, quad_capacity nodes of room */
  uint32_t quad_capacity;
  uint32_t reinsert_ran, passes, moves, undone;  /* stage 2: whether it ran (flag set, tree at or above the threshold), passes kept, moves applied */
  uint64_t visits;                               /* nodes its searches looked at, over all passes */
  double cost_before, cost_after;                /* pbrt_hip_scene_optimize_cost's sums */
  uint32_t dp_ran, n_quads, stack_need;
} pbrt_hip_build_stages;
#define PBRT_HIP_BUILD_STAGES_REINSERT 1u
/* Uploads the soup to `device`, runs the builder a scene is built with (gpu_build_quads; flags: PBRT_HIP_BUILD_STAGES_REINSERT = with stage 2,
 * as the default scene) with an observer that copies the tree to the host after every stage, and returns the copies.  No scene, no kernel
 * of its own.  PBRT_HIP_ERR_INVALID for a null P / idx / out, n_tris < 2, a vertex index >= n_verts, a vertex that is not finite. */
int pbrt_hip_gpu_build_stages_device(int device, const float *P, uint32_t n_verts, const uint32_t *idx, uint32_t n_tris, uint32_t flags,
                                     pbrt_hip_build_stages *out);
/* host only: stage 2 on a GIVEN tree -- child / boxes / order as above -> the link form after reinsert_batch_links with the default
 * ReinsertBatchParams (the device loop's passes, pbrt_amd/csrc/reinsert_batch.cpp), child order included.  stats (8 words): passes run (an
 * undone one included), visits, searches that found a move, moves applied, most visits of one search, undone, the summed area before and
 * after in fixed point, units of 2^-*fixed_exp (ri_cost_kernel's sums); *valid = LinkTree::valid of the result.  Outputs may be NULL.
 * PBRT_HIP_ERR_INVALID for a null input, n_tris < 2, a box that is not finite, a triangle id >= n_tris, a child word out of range or words
 * that do not form one tree. */
int pbrt_hip_reinsert_links_host(uint32_t n_tris, const uint32_t *child, const float *boxes, const uint32_t *order, uint32_t *par, uint32_t *kid,
                                 float *links_boxes, uint64_t *stats, int32_t *fixed_exp, uint32_t *valid);
/* host only: stage 3 on a GIVEN tree -- quad_nodes.cpp's collapse with the rule forced; a leaf child's slot is the tree's own.  Refusals as above,
 * and an unknown rule; PBRT_HIP_ERR_LIMIT when cap_nodes is too small. */
#define PBRT_HIP_COLLAPSE_GREEDY 1u
#define PBRT_HIP_COLLAPSE_DP 2u
int pbrt_hip_collapse_host(uint32_t n_tris, const uint32_t *child, const float *boxes, const uint32_t *order, uint32_t rule, uint32_t *quads,
                           uint32_t cap_nodes, uint32_t *n_quads, uint32_t *stack_need);

/* ---- samplers: the reference holds the Sobol' generator matrices (sobolmatrices.rs:81) and no sampler ---- */
/* host only: the generator matrices sampler 2 uses -- 128 dimensions x 32 columns, rows 0 .. 127 of the reference's
 * SOBOL_MATRICES32 (sobolmatrices.rs:81), the first 32 of its 52 columns -- for tests of that claim */
void pbrt_hip_sobol_matrices(uint32_t *out_4096_words);
/* ---- environment maps (pbrt_amd/csrc/envmap_core.hpp is the one statement of the arithmetic) ---- */
/* host only: the importance-sampling tables of an image (rgb: 3 x width x height, row 0 = theta 0): marginal = the CDF over rows (height
 * + 1 floats), conditional = one CDF per row (height x (width + 1) floats), p_uv = the density over (u, v) of every texel (width x
 * height floats: f / mean(f), f = luminance x sin(pi (row + 1/2) / height); a map that is black everywhere: f = the sine alone).  Any
 * output may be NULL.  The image is validated as pbrt_hip_scene_create validates it. */
int pbrt_hip_envmap_tables(const float *rgb, uint32_t width, uint32_t height, float *marginal, float *conditional, float *p_uv);
/* host only: envmap_core.hpp over arrays.  u12 != NULL: SAMPLE -- n pairs (u1, u2) in [0, 1) -> d (3 n floats, written), texel (row x
 * width + col of the texel drawn), le (its rgb, 3 n), pdf (the density over solid angle).  u12 == NULL: LOOKUP -- d (3 n, read) -> texel,
 * le, pdf of each direction.  texel, le, pdf may be NULL. */
int pbrt_hip_envmap_eval_host(const float *rgb, uint32_t width, uint32_t height, const float world_to_light[9], int64_t n, const float *u12,
                              float *d, uint32_t *texel, float *le, float *pdf);
/* the same on the device of `scene`, over the map and tables the scene holds (a tiny kernel that calls the same header): the same bits.
 * PBRT_HIP_ERR_INVALID for a scene without an environment map. */
int pbrt_hip_envmap_eval_device(pbrt_hip_scene *scene, int64_t n, const float *u12, float *d, uint32_t *texel, float *le, float *pdf);

/* ---- the kernels' building blocks (pbrt_amd/csrc/cephes_poly.hpp, kernel_math.hpp, envmap_core.hpp,
 * kernel_walk.hpp, tri_test.inc) ---- */
/* The production functions over arrays on `device`, one element per thread of a tiny kernel that calls the headers the render kernels
 * are built from (pbrt_amd/csrc/kernels_blocks.hip): what lets tests compare each of them with float64 and with the oracle's
 * restatement, element by element.  in / out are HOST arrays of n elements; the hook copies them in and out on the device's default
 * stream.  Floats per element, in -> out:
 *   SIN, COS, ATAN_POS, ACOS   x -> poly_sin / poly_cos / poly_atan_pos / poly_acos
 *   SINCOS                     x -> s, c of envmap::sincos_0_2pi
 *   SPHERE_UV                  nx ny nz -> u, v
 *   FRESNEL                    ci, r = eta_i / eta_t -> F, ct
 *   COSINE_ABOUT               n (3), u1, u2 -> wi (3), z
 *   SPHERE_HIT                 {centre, radius} (4), o (3), d (3), tmax -> hit (0 or 1), t (0 on a miss): sphere_hit alone, before the
 *                              own-box rule the walk applies to what it returns
 *   QUAD_STEP, QUAD_STEP_PK    the node's 16 words (raw bits in the float array), o (3), d (3), inv_parallel, tfar -> tn of children 0 .. 3,
 *                              the hit mask (bit k = child k), the slot entered (4 = none): one step of the production walk (kernel_walk.hpp
 *                              quad_step with the scalar and with the packed fma, the stand-in for 1 / 0 and the child selection around it)
 *   TRI_HIT                    p0 p1 p2 (9), o (3), d (3), tmax -> valid (0 or 1), t, u, v (zeros on a miss): the leaf pass's triangle test
 *                              (tri_test.inc: Moeller-Trumbore, the |det| cut, the own-box rule, t = max(th, entry))
 *   MIS_W_LIGHT, MIS_W_BSDF    pl, pb -> the power heuristic's weight of the light sample, pl^2 / (pl^2 + pb^2), and of the BSDF-sampled ray,
 *                              pb^2 / (pb^2 + pl^2) (kernel_math.hpp mis_weight_light / mis_weight_bsdf)
 *   LIGHT                      the light's five float4 records as the scene's light table holds them (20 floats: word 0 = the raw bits of the
 *                              device type -- 0 point, 1 distant, 2 constant sky, 3 emissive triangle --, words 1 .. 3 = p0; a triangle: 4 .. 6 =
 *                              p1, 7 = area, 8 .. 10 = p2, 16 .. 18 = unit normal; 12 .. 14 = the colour), po (3), nf (3), kd (3), u1, u2, nL as
 *                              a float, mis (0 or 1) -> accepted (0 or 1), Ld (3), wi (3), tmax (zeros where the light is ruled out): one call of
 *                              kernel_path.hpp sample_light, mis handed in as the literal the render kernels hand in
 * PBRT_HIP_ERR_INVALID for an unknown op, a negative n or a null array. */
#define PBRT_HIP_BLOCK_SIN 0u
#define PBRT_HIP_BLOCK_COS 1u
#define PBRT_HIP_BLOCK_ATAN_POS 2u
#define PBRT_HIP_BLOCK_ACOS 3u
#define PBRT_HIP_BLOCK_SINCOS 4u
#define PBRT_HIP_BLOCK_SPHERE_UV 5u
#define PBRT_HIP_BLOCK_FRESNEL 6u
#define PBRT_HIP_BLOCK_COSINE_ABOUT 7u
#define PBRT_HIP_BLOCK_SPHERE_HIT 8u
#define PBRT_HIP_BLOCK_QUAD_STEP 9u
#define PBRT_HIP_BLOCK_QUAD_STEP_PK 10u
#define PBRT_HIP_BLOCK_TRI_HIT 11u
#define PBRT_HIP_BLOCK_MIS_W_LIGHT 12u
#define PBRT_HIP_BLOCK_MIS_W_BSDF 13u
#define PBRT_HIP_BLOCK_LIGHT 14u
#define PBRT_HIP_BLOCK_COUNT 15u
int pbrt_hip_blocks_eval_device(int device, uint32_t op, int64_t n, const float *in, float *out);

/* ---- shading normals (pbrt_amd/csrc/shading_normal.inc is the one statement of the arithmetic) ---- */
/* The text the NRM render kernels include at a triangle hit, over arrays on `device` (a tiny kernel of kernels_n.hip that includes the same
 * file).  Floats per element, in (17): the corner normals n0 n1 n2 (9), the winding's unit normal ng (3), the barycentrics b1, b2, wo (3);
 * out (4): nsf (3) -- the interpolated, normalised normal turned to ng's side and then to wo's geometric side --, fell_back (0 or 1: the
 * interpolated normal was zero or not finite, nsf is +-ng bit for bit).  in / out are HOST arrays; PBRT_HIP_ERR_INVALID for a negative
 * n or a null array. */
int pbrt_hip_shading_normal_eval_device(int device, int64_t n, const float *in, float *out);

/* ---- weighted pixel filters (pbrt_amd/csrc/filter_weight.inc is the one statement of the arithmetic) ---- */
/* The footprint and table-index statements of the render kernels' weighted finish over arrays on `device` (two tiny kernels of
 * kernels_blocks.hip that call the same functions), for radii rx, ry and the cropped window crop = {x0, y0, x1, y1}:
 *   n_points film points (2 floats each) -> bounds, 4 ints each: x0, y0, x1, y1 of the footprint clipped to the window (x1, y1 exclusive);
 *   n_pairs (film point, pixel) pairs (2 floats, 2 ints each) -> index: iy * 16 + ix into the filter table, or -1 for a pixel outside the point's
 *   clipped footprint.
 * in / out are HOST arrays; either half may be empty (n = 0).  PBRT_HIP_ERR_INVALID for a negative n, a null array or radii that are
 * not positive and finite. */
int pbrt_hip_filter_footprint_eval_device(int device, float rx, float ry, const int32_t crop[4], int64_t n_points, const float *points,
                                          int32_t *bounds, int64_t n_pairs, const float *pair_points, const int32_t *pair_pixels, int32_t *index);

/* ---- image textures for Kd (pbrt_amd/csrc/image_lookup.hpp is the one statement of the arithmetic) ---- */
/* host only: the lookup of record `which` of `records` (n_records >= 1 records of type 4, checked as pbrt_hip_scene_create checks them and
 * packed into ONE texel pool as it packs them) at n points: uv = (u, v) pairs, 2 n floats -> rgb, 3 n floats = Kd, the record's mapping
 * (s, t) = (su u + du, sv v + dv) included. */
int pbrt_hip_image_lookup_eval_host(const pbrt_hip_image_texture *records, uint32_t n_records, uint32_t which, int64_t n, const float *uv, float *rgb);
/* the same on `device` (a tiny kernel of kernels_blocks.hip that calls the same header over the uploaded pool): the same bits.
 * PBRT_HIP_ERR_NO_DEVICE without one. */
int pbrt_hip_image_lookup_eval_device(int device, const pbrt_hip_image_texture *records, uint32_t n_records, uint32_t which, int64_t n, const float *uv,
                                      float *rgb);

/* ---- the plastic material's BSDF (pbrt_amd/csrc/plastic_bsdf.hpp is the one statement of the arithmetic) ---- */
/* plastic_bsdf.hpp over arrays on `device` (a small kernel of kernels_blocks.hip): element i reads 18 floats of `in` -- nf, wo, wi (unit
 * vectors, nf the normal turned towards wo), u1, u2, Kd.rgb, Ks.rgb, alpha -- and writes 10 floats of `out`: f(wo, wi).rgb, pdf_b(wi), the
 * direction wi' the sampler draws from (u1, u2), and f(wo, wi') cos / pdf_b(wi').rgb (the last six are zero where the sample dies).  in /
 * out are HOST arrays.  PBRT_HIP_ERR_INVALID for a negative n or a null array, PBRT_HIP_ERR_NO_DEVICE without a device. */
#define PBRT_HIP_PLASTIC_EVAL_IN 18
#define PBRT_HIP_PLASTIC_EVAL_OUT 10
int pbrt_hip_plastic_eval_device(int device, int64_t n, const float *in, float *out);

/* ---- the substrate material's BSDF (pbrt_amd/csrc/substrate_bsdf.hpp is the one statement of the arithmetic) ---- */
/* substrate_bsdf.hpp over arrays on `device` (a small kernel of kernels_blocks.hip), in pbrt_hip_plastic_eval_device's layout: 18 floats
 * in -- nf, wo, wi, u1, u2, Kd.rgb, Ks.rgb, alpha --, 10 floats out -- f(wo, wi).rgb, pdf_b(wi), the sampled wi', f(wo, wi') cos /
 * pdf_b(wi').rgb (the last six zero where the sample dies).  in / out are HOST arrays.  The same refusals. */
#define PBRT_HIP_SUBSTRATE_EVAL_IN 18
#define PBRT_HIP_SUBSTRATE_EVAL_OUT 10
int pbrt_hip_substrate_eval_device(int device, int64_t n, const float *in, float *out);

/* ---- the spot light's sample (pbrt_amd/csrc/spot_light.hpp is the one statement of the arithmetic) ---- */
/* spot_light.hpp over arrays on `device` (a small kernel of kernels_blocks.hip): element i reads 15 floats of `in` -- the shading point po,
 * its normal nf, the light's position p, the cone's axis, cos_total, cos_start, nL (the scene's light count as a float) -- and writes 7
 * floats of `out`: ok (1 or 0), wi.xyz, tmax, the falloff, and scale = ((cos / dist^2) nL) falloff (the last six are zero where ok is).
 * in / out are HOST arrays.  PBRT_HIP_ERR_INVALID for a negative n or a null array, PBRT_HIP_ERR_NO_DEVICE without a device. */
#define PBRT_HIP_SPOT_EVAL_IN 15
#define PBRT_HIP_SPOT_EVAL_OUT 7
int pbrt_hip_spot_eval_device(int device, int64_t n, const float *in, float *out);

/* ---- a mapped light's sample (pbrt_amd/csrc/light_map.hpp is the one statement of the arithmetic) ---- */
/* light_map.hpp over arrays on `device` (a small kernel of kernels_blocks.hip) for ONE light-map record and the image it reads (the
 * record's own `image` number is not used): element i reads 10 floats of `in` -- the shading point po, its normal nf, the light's position
 * p, nL (the scene's light count as a float) -- and writes 11 floats of `out`: ok (1 or 0), wi.xyz, tmax, scale = (cos / dist^2) nL, the
 * image coordinates s, t, and the image's rgb there (the last ten are zero where ok is).  in / out are HOST arrays.  Both records are checked
 * as scene creation checks them (PBRT_HIP_ERR_INVALID / _LIMIT); PBRT_HIP_ERR_INVALID for a negative n or a null pointer. */
#define PBRT_HIP_LIGHT_MAP_EVAL_IN 10
#define PBRT_HIP_LIGHT_MAP_EVAL_OUT 11
int pbrt_hip_light_map_eval_device(int device, const pbrt_hip_image_texture *image, const pbrt_hip_light_map *map, int64_t n, const float *in, float *out);

/* ---- a sphere light's sample (pbrt_amd/csrc/sphere_light.hpp is the one statement of the arithmetic) ---- */
/* sphere_light.hpp over arrays on `device` (a small kernel of kernels_blocks.hip): element i reads 13 floats of `in` -- the shading point
 * po, its normal nf, the sphere's centre c and radius r, the pair u1 u2, nL (the scene's light count as a float) -- and writes 8 floats of
 * `out`: ok (1 or 0), wi.xyz, tmax, scale = cos (1 / pdf_omega) nL, pdf_omega (these six are zero where ok is), and the hit side's
 * pdf_omega from po (0 where po is not outside the sphere; it does not depend on ok).  in / out are HOST arrays.  PBRT_HIP_ERR_INVALID for
 * a negative n or a null array, PBRT_HIP_ERR_NO_DEVICE without a device. */
#define PBRT_HIP_SPHERE_LIGHT_EVAL_IN 13
#define PBRT_HIP_SPHERE_LIGHT_EVAL_OUT 8
int pbrt_hip_sphere_light_eval_device(int device, int64_t n, const float *in, float *out);

/* ---- the small device tables of a scene, as scene creation assembles them on the host (pbrt_amd/csrc/scene_tables.hpp states their rows) ---- */
/* HOST arrays of 32-bit words that pbrt_hip_scene_tables_host fills, each of which may be NULL, and beside each the count of words it holds
 * (set whether or not the array is given: a first call with every array NULL sizes a second one).  P / idx / mat: the primitives the tree
 * builders get -- the triangles, then the spheres' proxy triangles; a material id is widened to a word.  lights, mats, mat_extra, spheres,
 * textures, image_texels: the kernels' tables, 4 words per row.  The scalars are the gather stage's. */
typedef struct pbrt_hip_scene_tables {
  uint32_t *P, *idx, *mat, *lights, *mats, *mat_extra, *spheres, *textures, *image_texels;
  uint32_t n_P, n_idx, n_mat, n_lights, n_mats, n_mat_extra, n_spheres, n_textures, n_image_texels;
  float le_inf[3];
  uint32_t has_inf, env, has_spot, has_mapped, env_w, env_h;
  float env_m[9], env_c[3];
} pbrt_hip_scene_tables;
/* host only, no HIP call (it works on a machine without a device): checks `desc` as pbrt_hip_scene_create does (the same refusals, flags 0)
 * and runs the gather stage on it.  PBRT_HIP_ERR_INVALID for a null argument. */
int pbrt_hip_scene_tables_host(const pbrt_hip_scene_desc *desc, pbrt_hip_scene_tables *out);

/* ---- the parser's state and its tokenizer alone (conformance tests replay parser.rs:778-880, api.rs:979-1045) ---- */
/* CTM (current_transform[0].m) when parsing stopped, and the directive names stored by the option setters
 * (api.rs:778-820) as "camera sampler integrator filter accelerator film" */
int pbrt_hip_loaded_state(const pbrt_hip_loaded *loaded, float ctm[16], char *names, size_t names_cap);
/* the tokenizer alone (parser.rs:61-170): tokens '\n'-separated into buf; returns the token count, or
 * -(1 + count) when the stream ends in an error (EOF / newline inside a quoted string) after `count` tokens */
int pbrt_hip_tokenize(const char *text, size_t len, char *buf, size_t cap);

#ifdef __cplusplus
}
#endif
#endif
