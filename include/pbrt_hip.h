/*
 * pbrt_hip.h -- C ABI of the MI355X render path ("what `PbrtAPI::world_end` calls").
 *
 * The reference (wathiede/pbrt, Rust) has no FFI layer and no renderer: the seam this
 * library fills is the body of `fn world_end(&mut self)` (/root/reference/src/core/api.rs:432-473,
 * whose render call survives only as the comment at :446-453), reached from the parser's
 * "WorldEnd" arm (src/core/parser.rs:312).  Its inputs are the fields of `RenderOptions`
 * (api.rs:201-224) -- camera_to_world (api.rs:813-820), film/sampler/integrator parameters --
 * plus the geometry the reference never stores (api.rs:220-223 TODO).  INTEGRATION.md shows the
 * `extern "C"` block and the `world_end` body a maintainer of the Rust crate would add.
 *
 * This header is what a host binds.  The hooks of tests and measurements (tree exports, walk / stack-plan introspection, the
 * host-only builders, the tokenizer alone, parser state) live in pbrt_hip_debug.h: same library, not part of the stable ABI.
 *
 * Conventions
 *  - plain pointers and sizes only; the caller owns every HOST pointer it passes, the library
 *    copies what it needs during the call and keeps nothing;
 *  - every function returns 0 on success or a negative pbrt_hip_status; the message is
 *    available from pbrt_hip_last_error() (thread-local); no C++ exception crosses the ABI
 *    (reference error style: api.rs:50-63 `Error`, api.rs:291-332 verify_* = log and continue);
 *  - there is NO CPU fallback: without a HIP device every entry point that computes returns
 *    PBRT_HIP_ERR_NO_DEVICE;
 *  - a scene handle is used by one host thread at a time (api.rs is single-threaded).
 */
#ifndef PBRT_HIP_H
#define PBRT_HIP_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
  PBRT_HIP_OK = 0,
  PBRT_HIP_ERR_INVALID = -1,   /* bad argument */
  PBRT_HIP_ERR_NO_DEVICE = -2, /* no HIP device / HIP runtime error at init */
  PBRT_HIP_ERR_HIP = -3,       /* a HIP call failed */
  PBRT_HIP_ERR_LIMIT = -4,     /* scene exceeds a compiled-in limit (BVH depth, material count) */
  PBRT_HIP_ERR_INTERNAL = -5
} pbrt_hip_status;

#define PBRT_HIP_MATERIAL_MATTE 0u
#define PBRT_HIP_MATERIAL_MIRROR 1u
#define PBRT_HIP_MATERIAL_GLASS 2u
#define PBRT_HIP_MATERIAL_PLASTIC 3u
#define PBRT_HIP_MATERIAL_SUBSTRATE 4u
/* Material "matte" / "mirror" / "glass" (scene files name them: scenes/check-sphere.pbrt:21,29; the
 * reference only has the TODO at api.rs:255-269).  32 bytes.
 * GLASS (type 2) is pbrt-v3's GlassMaterial with zero roughness: one FresnelSpecular lobe, an interface between index 1
 * on the side the geometric normal points to (a triangle's winding normal, a sphere's outward one) and index eta on the other; no
 * nested media.  It needs seven numbers and reuses the seven words after `type`:
 *   k = Kr (reflectance), le = Kt (TRANSMITTANCE -- a glass surface does not emit), kd_tex = the IEEE-754 bits of the float eta.
 * Kr, Kt finite and >= 0, eta finite and in [1, 16] (PBRT_HIP_ERR_INVALID otherwise, the message holds "glass").  At a hit ONE 1-D
 * sample chooses reflection (probability F, the Fresnel reflectance; weight Kr) or refraction (1 - F; weight Kt eta_i^2 / eta_t^2:
 * radiance transport); also under Integrator "directlighting", where pbrt-v3 follows both branches and this path follows the one
 * chosen (same expectation).  Every interface crossed costs one bounce of max_depth.  A glass primitive occludes shadow rays (as in
 * pbrt-v3: no caustics by light sampling).  Not with the counter flags (PBRT_HIP_ERR_LIMIT).
 * PLASTIC (type 3) is pbrt-v3's PlasticMaterial: a Lambertian base Kd / pi plus a Trowbridge-Reitz microfacet reflection of
 * isotropic width alpha with the Fresnel term of a dielectric of index 1.5 against 1.  It reuses the record the way glass does:
 *   k = Kd, le = Ks (a plastic surface does not emit), kd_tex = the IEEE-754 bits of the float alpha.
 * Kd, Ks finite and >= 0, alpha finite and in [1e-3, 1] (PBRT_HIP_ERR_INVALID otherwise, the message holds "plastic"; a type-3 record whose
 * le and kd_tex are all zero -- nothing of plastic in it -- is refused as "unknown material type", as every type-3 record was until 0.10).  A plastic vertex
 * draws what a matte one draws, in the same order; its lobe is about the GEOMETRIC normal.  Rendered for every integrator, sampler and
 * filter, with spheres, textures on other materials, glass; NOT in a scene whose texture table holds an environment map (slot type 1) or
 * shading normals (slot type 2): pbrt_hip_scene_create refuses the pair with PBRT_HIP_ERR_LIMIT (the message holds "plastic").  Not with
 * the counter flags (PBRT_HIP_ERR_LIMIT at render, as for glass).
 * SUBSTRATE (type 4) is pbrt-v3's SubstrateMaterial, a FresnelBlend BSDF: a diffuse base Kd (1 - Ks) that darkens at grazing
 * angles under a glossy coat, one Trowbridge-Reitz lobe of isotropic width alpha with Schlick's Fresnel term on Ks and no masking term.  The
 * record is reused as plastic reuses it:
 *   k = Kd, le = Ks (a substrate surface does not emit), kd_tex = the IEEE-754 bits of the float alpha.
 * Kd finite and >= 0, Ks finite and in [0, 1] (beyond 1 the factor 1 - Ks makes the BSDF negative), alpha finite and in [1e-3, 1]
 * (PBRT_HIP_ERR_INVALID otherwise, the message holds "substrate").  A substrate vertex draws what a plastic one draws, in the same order,
 * from the same direction sampler; it is rendered where plastic is and refused where plastic is (PBRT_HIP_ERR_LIMIT beside an environment
 * map or shading normals, the message holds "substrate"; the counter flags as for glass).  Type 5 and above are unknown material types. */
typedef struct {
  uint32_t type; /* PBRT_HIP_MATERIAL_*: 0 = matte (Lambertian, k = Kd), 1 = mirror (perfect specular, k = Kr), 2 = glass, 3 = plastic, 4 = substrate (above) */
  float k[3];
  float le[3]; /* emitted radiance; non-zero turns every triangle using it into an area light
                  (replaces api.rs:476-478 area_light_source -> todo!()).  GLASS: Kt.  PLASTIC, SUBSTRATE: Ks */
  uint32_t kd_tex; /* GLASS: the bits of the float eta.  PLASTIC, SUBSTRATE: the bits of the float alpha.  Matte only: 0 = Kd is k; t > 0 = Kd is textures[t - 1] evaluated at the hit's (u, v): a triangle's corner (u, v)
                      (tri_uv) interpolated like the hit point; a SPHERE's own (u, v) = (phi / 2 pi, 1 - theta / pi) with phi = atan2(n.y, n.x)
                      in [0, 2 pi), theta = acos(n.z) of the unit normal n about the WORLD's z axis (pbrt-v3 Sphere::Intersect for an
                      unrotated sphere: a sphere here is a centre and a radius, its CTM's rotation is not carried -- the parser warns) */
} pbrt_hip_material;

/* Texture "name" "spectrum" "checkerboard" (check-sphere.pbrt:24-25; the reference: api.rs:524-580 stores nothing, texture.rs is an
 * empty marker): pbrt-v3's Checkerboard2DTexture over a UVMapping2D, point-sampled (aamode "none": no ray differentials here):
 * (s, t) = (su u + du, sv v + dv); tex1 where floor(s) + floor(t) is even, tex2 where odd.  64 bytes. */
typedef struct {
  uint32_t type;  /* 0 = checkerboard, dimension 2, "uv" mapping; 1 = this slot is the environment-map record below; 2 = the shading
                     normals' record, pbrt_hip_normals; 3 = the pixel filter's record, pbrt_hip_pixel_filter; 4 = an image texture's
                     record, pbrt_hip_image_texture; 6 = a spot light's cone, pbrt_hip_spot_cone; 8 = a mapped light's record,
                     pbrt_hip_light_map */
  float tex1[3], tex2[3];
  float su, sv, du, dv; /* "float uscale" / "vscale" / "udelta" / "vdelta" */
  uint32_t pad[5];
} pbrt_hip_texture;

/* Texture "name" "spectrum" "imagemap" (the reference stores no texture, api.rs:524-580): pbrt-v3's ImageTexture over a
 * UVMapping2D without a MIPMap pyramid -- a matte Kd read from an image.  A slot of `textures` whose first word is 4 IS this record -- 64
 * bytes, read with memcpy like the environment map's; a matte kd_tex = t names it exactly as it names a checkerboard, and the hit's (u, v)
 * and (s, t) = (su u + du, sv v + dv) are the checkerboard's own.  t = 0 is the BOTTOM row of the image (pbrt-v3): texel row iy counts
 * from the bottom and is row height - 1 - iy of `rgb`.  All arithmetic in fp32; an index stays a float until it is clamped to [0, W - 1]
 * (NaN -> 0), so every s has a defined texel.
 *   filter 0 point     repeat: ix = floor((s - floor(s)) W); clamp, black: ix = floor(s W), clamped; black: 0 outside [0, W - 1]
 *   filter 1 bilinear  texel centres at (i + 0.5) / W (MIPMap::Lookup at level 0 without ray differentials): repeat reduces s - floor(s)
 *                      first; sx = s W - 0.5, x0 = floor(sx), the four neighbours weighted (1 - dx, dx) x (1 - dy, dy); repeat wraps a
 *                      neighbour, clamp clamps it, black gives it weight 0 outside
 * Refused at scene creation before any device work (the message holds "image"): width or height 0, a NULL `rgb`, a texel that is not finite
 * or is negative, an unknown wrap / filter, a mapping that is not finite (PBRT_HIP_ERR_INVALID); width or height > 16384, more than 64 image
 * slots, more than 2^26 texels in all of them (PBRT_HIP_ERR_LIMIT).  A scene with an image-textured material is a textured scene: the
 * kernels, the refusals (counter flags: PBRT_HIP_ERR_LIMIT) and tri_uv are the checkerboard's.  Glass ignores kd_tex as before. */
#define PBRT_HIP_TEXTURE_IMAGE 4u
#define PBRT_HIP_WRAP_REPEAT 0u
#define PBRT_HIP_WRAP_CLAMP 1u
#define PBRT_HIP_WRAP_BLACK 2u
#define PBRT_HIP_TEXFILTER_POINT 0u
#define PBRT_HIP_TEXFILTER_BILINEAR 1u
#define PBRT_HIP_IMAGE_MAX_SIZE 16384u        /* width, height */
#define PBRT_HIP_IMAGE_MAX_SLOTS 64u
#define PBRT_HIP_IMAGE_MAX_TEXELS (1u << 26)  /* all image slots of a scene together */
typedef struct {
  uint32_t type;     /* = 4 */
  uint32_t width, height;
  uint32_t wrap;     /* PBRT_HIP_WRAP_*: 0 repeat, 1 clamp, 2 black */
  const float *rgb;  /* host, 3 x width x height, row-major, row 0 = the first row pbrt_hip_read_image returns (the image's top); copied
                        during the call */
  float su, sv, du, dv; /* "float uscale" / "vscale" / "udelta" / "vdelta" */
  uint32_t filter;   /* PBRT_HIP_TEXFILTER_*: 0 point, 1 bilinear */
  uint32_t pad[5];
} pbrt_hip_image_texture;

/* LightSource "infinite" "string mapname" (the reference: src/lights/infinite.rs:52-66 reads the image, multiplies the
 * texels by L x scale and stops at todo!() before its MIPMap and Distribution2D): an environment map in the latitude-longitude
 * parametrisation of pbrt-v3's InfiniteAreaLight.  A slot of `textures` whose first word is 1 IS this record -- also 64 bytes; the table's
 * element type is 4-aligned, so the library reads the slot with memcpy, and a host may fill it the same way.
 *   direction d -> w = world_to_light d, phi = atan2(w.y, w.x) in [0, 2 pi), theta = acos(w.z), (u, v) = (phi / 2 pi, theta / pi),
 *   col = min((int)(u width), width - 1), row = min((int)(v height), height - 1); row 0 of `rgb` -- the first row pbrt_hip_read_image
 *   returns -- is theta = 0, the light's +z.
 * POINT-SAMPLED, as the checkerboard is: Le(d) = c x texel[row][col] (c: the light's factor, below), a piecewise-constant sky -- a deliberate
 * difference from pbrt-v3's bilinear MIPMap::Lookup, which makes the sampling density exactly proportional to the radiance it samples.
 * The light is importance-sampled by pbrt-v3's Distribution2D over luminance x sin theta, from the same (u1, u2) every other light gets.
 * Refused before any device work (the message holds "environment"): width x height > 2^24 (PBRT_HIP_ERR_LIMIT); width or height 0, a NULL
 * `rgb`, a texel that is not finite or is negative, a world_to_light that is not finite or not orthonormal to 1e-4
 * (PBRT_HIP_ERR_INVALID); a matte kd_tex that names such a slot (PBRT_HIP_ERR_INVALID: a texture for Kd is a slot of type 0 or 4). */
typedef struct {
  uint32_t type;     /* = 1 */
  uint32_t width, height;
  uint32_t reserved; /* = 0 */
  const float *rgb;  /* host, 3 x width x height, row-major, copied during the call */
  float world_to_light[9]; /* row-major 3 x 3 rotation: the inverse of the light's CTM */
  uint32_t pad;
} pbrt_hip_envmap;

/* Shape "trianglemesh" "normal N" / "plymesh" with nx ny nz and "bool shadingnormals" "true" (the reference reads neither): per-corner shading normals.
 * A slot of `textures` whose first word is 2 IS this record -- 64 bytes, read with memcpy like the environment map's.  At a triangle hit
 * the three corner normals are interpolated with the hit's barycentrics in the order of the hit point, normalised and turned to the side
 * of the WINDING's normal ng (pbrt-v3 turns ng towards N instead: a deliberate difference -- one-sided emission and everything else that
 * hangs on ng stays where it was); matte and mirror scatter about that shading normal, a light sample and a bounce count only on the
 * geometric front side as well.  A triangle whose interpolated normal is zero (all three corners zero = "this mesh has none") or not
 * finite is shaded flat.  Spheres keep their analytic normal; a GLASS triangle ignores its normals (3.16 keeps ng).
 * Refused before any device work (the message holds "normal"): more than one such slot (PBRT_HIP_ERR_LIMIT); n_tris other than the
 * description's, a NULL tri_n, a component that is not finite, a matte kd_tex that names the slot (PBRT_HIP_ERR_INVALID).  A scene with the
 * slot runs the NRM kernels (kernels_n.hip render_kernel_n); they exist for every integrator and sampler, with and without spheres,
 * textures, glass and an environment map, and NOT for: a box filter radius other than 0.5, the counter flags (both PBRT_HIP_ERR_LIMIT at
 * render, the message names the combination). */
#define PBRT_HIP_TEXTURE_NORMALS 2u
typedef struct {
  uint32_t type;        /* = 2 */
  uint32_t n_tris;      /* must equal desc.n_tris */
  uint32_t reserved[2]; /* = 0 */
  const float *tri_n;   /* host, 9 * n_tris: the normals of the three corners of every triangle, world space, any length; a zero
                           normal = "none"; copied during the call */
  uint32_t pad[10];
} pbrt_hip_normals;

/* PixelFilter "triangle" / "gaussian" / "mitchell" / "sinc" (pbrt-v3's TriangleFilter, GaussianFilter, MitchellFilter,
 * LanczosSincFilter and FilmTile::AddSample; the reference builds Film's 16 x 16 filter table, film.rs:113-123, and has nothing that
 * uses it).  A slot of `textures` whose first word is 3 IS this record -- 64 bytes, read with memcpy like the environment map's.  The box
 * is not a kind: a scene without the record is filtered as before.  With the record, pbrt_hip_render_desc.filter_xwidth / ywidth stay the
 * radii rx, ry (0 = the kind's default: 2 x 2 for kinds 1 .. 3, 4 x 4 for kind 4), and a sample at film point p adds w x L to every pixel
 * (x, y) of the cropped window with |x + 0.5 - p.x| <= rx, |y + 0.5 - p.y| <= ry -- the box's footprint --, w from the 16 x 16 table of
 * pbrt_hip_filter_table.  The film is the fixed-point film of every wide filter (pbrt_hip_render_acc below) at EVERY radius, 0.5
 * included; its fourth accumulator is the sum of the weights in units of 2^-24, not a sample count.
 *   kind 1 triangle   max(0, rx - |x|) max(0, ry - |y|)
 *   kind 2 gaussian   g(x, rx) g(y, ry), g(d, r) = max(0, exp(-alpha d^2) - exp(-alpha r^2)); param[0] = alpha (pbrt-v3's default: 2)
 *   kind 3 mitchell   M(x / rx) M(y / ry), M of pbrt-v3's Mitchell1D; param[0] = B, param[1] = C (1/3 each)
 *   kind 4 sinc       W(x, rx) W(y, ry), W(x, r) = 0 beyond r, else sinc(|x|) sinc(|x| / tau), sinc(x) = 1 below 1e-5, else
 *                     sin(pi x) / (pi x); param[0] = tau (3)
 * Refused at scene creation before any device work (the message holds "filter"): more than one such slot (PBRT_HIP_ERR_LIMIT); an unknown
 * kind, a parameter that is not finite, alpha <= 0 or tau <= 0, a matte kd_tex that names the slot (PBRT_HIP_ERR_INVALID).  A render is a
 * wide-filter render: not with an environment map, shading normals or the counter flags, and refused with PBRT_HIP_ERR_LIMIT when spp x
 * footprint x ceil(largest |table entry|) passes 2^24 (the accumulators could wrap). */
#define PBRT_HIP_TEXTURE_FILTER 3u
#define PBRT_HIP_FILTER_TRIANGLE 1u
#define PBRT_HIP_FILTER_GAUSSIAN 2u
#define PBRT_HIP_FILTER_MITCHELL 3u
#define PBRT_HIP_FILTER_SINC 4u
typedef struct {
  uint32_t type;  /* = 3 */
  uint32_t kind;  /* PBRT_HIP_FILTER_*: 1 .. 4 */
  float param[2]; /* gaussian: alpha; mitchell: B, C; sinc: tau; the others 0 */
  uint32_t pad[12];
} pbrt_hip_pixel_filter;

/* LightSource "point" / "distant" / "infinite" (api.rs:334-351 make_light: todo!() for all).
 * Type 3 is the infinite light with an environment map: c = the factor on the texels (L x scale, infinite.rs:54), `pad`
 * = the BITS of the 1-based number of a type-1 slot of `textures` (the way glass keeps eta in kd_tex), p is ignored.  A type-3 light
 * that names no such slot is PBRT_HIP_ERR_INVALID, more than one type-3 light PBRT_HIP_ERR_LIMIT (messages hold "environment").
 * Constant infinite lights (type 2) work beside it.  A scene with a map runs the ENV kernels (kernels_env.hip render_kernel_env); they
 * exist for every integrator and sampler, with and without spheres, textures and glass, and NOT for: a box filter radius other than
 * 0.5, the counter flags (both PBRT_HIP_ERR_LIMIT at render, the message names the combination). */
#define PBRT_HIP_LIGHT_ENVMAP 3u
/* LightSource "spot" (pbrt-v3's SpotLight): type 5 -- 4 stays an unknown light type --, a point light at p with intensity c
 * = I inside a cone with a smooth edge.  The 32-byte record cannot hold the cone, so `pad` = the BITS of the 1-based number of a type-6 slot
 * of `textures` -- a pbrt_hip_spot_cone record, named the way the environment map's light names its map --: a unit axis that points AWAY from the light and
 * two cosines cos_total <= cos_start.  For a shading point with unit direction wi towards the light, ct = -(wi . axis):
 *   falloff = 0 where ct < cos_total, 1 where ct >= cos_start, else ((ct - cos_total) / (cos_start - cos_total))^4
 * and the light is the point light times that falloff; cos_total = cos_start is a hard edge.  A delta light: MIS weight 1, never hit by a
 * ray.  Several spot lights may share a cone slot.  Refused at scene creation before any device work (PBRT_HIP_ERR_INVALID, the message
 * holds "spot"): a type-5 light whose `pad` names no type-6 slot; an axis that is not finite or whose squared length is off 1 by more than
 * 1e-4; a cosine that is not finite or lies outside [-1, 1]; cos_total > cos_start; a matte kd_tex that names a cone slot.  A scene with a
 * spot light is rendered by the kernels that render glass and plastic (the GLS instantiations of render_kernel_x), for every integrator,
 * sampler and filter; NOT in a scene whose texture table holds an environment map (slot type 1) or shading normals (slot type 2):
 * pbrt_hip_scene_create refuses the pair with PBRT_HIP_ERR_LIMIT (the message holds "spot").  Not with the counter flags
 * (PBRT_HIP_ERR_LIMIT at render, as for glass). */
#define PBRT_HIP_LIGHT_SPOT 5u
#define PBRT_HIP_TEXTURE_SPOT 6u /* (slot types 5 and 7 stay unknown texture types) */
typedef struct {
  uint32_t type;   /* = 6 */
  float axis[3];   /* unit, world space, from the light into the cone */
  float cos_total; /* cosine of the cone's half angle: no light outside */
  float cos_start; /* cosine of the angle at which the falloff starts: full intensity inside; >= cos_total */
  uint32_t pad[10];
} pbrt_hip_spot_cone;
/* LightSource "projection" / "goniometric" (pbrt-v3's ProjectionLight and GonioPhotometricLight): type 6 -- 4 and 7 stay
 * unknown light types --, a point light at p with intensity c = I, multiplied by an image looked up in the direction from the light to
 * the shaded point.  `pad` = the BITS of the 1-based number of a type-8 slot of `textures`, a pbrt_hip_light_map record:
 *   kind            0 projection, 1 goniometric
 *   image           the 1-based number of a type-4 slot (pbrt_hip_image_texture): its texels, wrap and filter serve the light; its su sv du dv
 *                   are ignored.  A material may name the same slot
 *   world_to_light  a row-major rotation, as pbrt_hip_envmap has it
 *   inv_tan, sx, sy projection: 1 / tan(fov / 2) and the half extents of the screen window; goniometric: all three 0
 * With wi the unit direction from the shaded point towards the light, d = -wi and w = world_to_light d:
 *   projection   (the light looks along its +z) no light unless w.z > 1e-3; px = (w.x / w.z) inv_tan, py = (w.y / w.z) inv_tan; no light
 *                unless -sx <= px <= sx and -sy <= py <= sy; (s, t) = ((px + sx) / (2 sx), (py + sy) / (2 sy))
 *   goniometric  (the light's +y is the pole, pbrt-v3's swap of y and z) theta = acos(clamp(w.y, -1, 1)), phi = atan2(w.z, w.x) in
 *                [0, 2 pi); (s, t) = (phi / 2 pi, 1 - theta / pi)
 * and the light is the point light times the image at (s, t), t = 0 the image's BOTTOM row: the file's top row is the light's +y of a
 * projection and the +y pole of a goniometric map (a deliberate choice: DESIGN.md 3.23).  No sample where all three channels are 0.  A delta
 * light: MIS weight 1, never hit by a ray.  Several lights may share a record.  Refused at scene creation before any device work
 * (PBRT_HIP_ERR_INVALID, the message holds "light map"): a type-6 light whose `pad` names no type-8 slot; a kind other than 0 or 1; an
 * `image` that names no type-4 slot; a world_to_light that is not finite or off orthonormal by more than 1e-4; projection: inv_tan, sx or
 * sy not finite or not > 0; goniometric: any of the three not 0; a matte kd_tex that names a type-8 slot.  A record no light names is held
 * to the same rules.  Rendered by the kernels that render glass, plastic and spot lights (the GLS instantiations of render_kernel_x), for
 * every integrator, sampler and filter; NOT in a scene whose texture table holds an environment map (slot type 1) or shading normals (slot
 * type 2): PBRT_HIP_ERR_LIMIT (the message holds "light map").  Not with the counter flags (PBRT_HIP_ERR_LIMIT at render, as for glass). */
#define PBRT_HIP_LIGHT_MAPPED 6u
#define PBRT_HIP_TEXTURE_LIGHT_MAP 8u /* (slot types 5 and 7 stay unknown texture types) */
#define PBRT_HIP_LIGHT_MAP_PROJECTION 0u
#define PBRT_HIP_LIGHT_MAP_GONIOMETRIC 1u
typedef struct {
  uint32_t type;  /* = 8 */
  uint32_t kind;  /* PBRT_HIP_LIGHT_MAP_* */
  uint32_t image; /* 1-based number of a type-4 slot */
  float world_to_light[9];
  float inv_tan, sx, sy;
  uint32_t pad[1];
} pbrt_hip_light_map;
/* AreaLightSource "diffuse" on a Shape "sphere" (pbrt-v3's DiffuseAreaLight over Sphere::Sample): type 8 -- 4 and 7 stay
 * unknown light types --, a light that NAMES a sphere of the scene: `pad` = the BITS of the sphere's 1-based number in `spheres`, c = the
 * radiance L, which must equal the `le` of that sphere's material bit for bit (the surface a ray hits and the light a vertex samples then
 * cannot disagree), p is not used (it must be finite, as every light's p must).  The named sphere is held to every sphere's
 * rules first: its radius is finite and positive before the light is looked at.  The sphere stays the primitive it is: camera rays and specular paths see its emission through the
 * material.  What the light adds is the direct-light estimate: a matte, plastic or substrate vertex samples the sphere uniformly in the
 * solid angle it subtends (one-sided, outward: a vertex inside the sphere gets nothing), and under MIS a BSDF-sampled ray that lands on the
 * sphere from outside carries the power heuristic's other half.  An emissive sphere that NO light names renders as it always did: seen
 * by camera rays and after specular bounces only.  Refused at scene creation before any device work (PBRT_HIP_ERR_INVALID, the message
 * holds "sphere light"): a `pad` that names no sphere; two lights that name one sphere; a sphere whose material is glass, plastic or
 * substrate (they reuse `le`); an `le` with no positive channel; a c that differs from `le`.  Rendered by the kernels that render glass,
 * plastic, spot and mapped lights (the GLS instantiations of render_kernel_x), for every integrator, sampler and filter; NOT in a scene
 * whose texture table holds an environment map (slot type 1) or shading normals (slot type 2): PBRT_HIP_ERR_LIMIT (the message holds
 * "sphere light").  Not with the counter flags (PBRT_HIP_ERR_LIMIT at render, as for glass). */
#define PBRT_HIP_LIGHT_SPHERE 8u
typedef struct {
  uint32_t type; /* 0 point, 1 distant, 2 infinite with constant radiance, 3 infinite with an environment map, 5 spot, 6 mapped, 8 sphere */
  float p[3];    /* point, spot, mapped: position; distant: unit direction TOWARDS the light */
  float c[3];    /* point, spot, mapped: intensity I; distant / infinite / sphere: radiance L; 3: the factor on the texels */
  float pad;     /* 3: the bits of the texture-table number (1-based) of the pbrt_hip_envmap; 5: of the pbrt_hip_spot_cone; 6: of the
                    pbrt_hip_light_map; 8: of the sphere's number (1-based) in `spheres` */
} pbrt_hip_light;

/* Shape "sphere" (check-sphere.pbrt:22), world space.  A primitive of the BVH like a triangle (primitive number n_tris + index, which is
 * what pbrt_hip_intersect reports), bounded by [c - r, c + r]: thousands of spheres cost a ray what thousands of triangles do. */
typedef struct {
  float c[3];
  float r;
  uint32_t mat;
  uint32_t pad[3];
} pbrt_hip_sphere;

/* Everything RenderOptions would hold at WorldEnd (api.rs:201-224), as arrays. */
typedef struct {
  const float *P;         /* "point P": 3 * n_verts (parser.rs:821-839 shows the param shape) */
  const uint32_t *idx;    /* "integer indices": 3 * n_tris */
  const uint16_t *mat_id; /* n_tris, index into mats */
  const pbrt_hip_material *mats;
  const pbrt_hip_light *lights;
  const pbrt_hip_sphere *spheres;
  uint32_t n_verts, n_tris, n_mats, n_lights, n_spheres;
  float cam_to_world[16]; /* RenderOptions.camera_to_world, row-major Matrix4x4 (transform.rs:75-77) */
  float fov;              /* Camera "perspective" "float fov" (degrees, shorter axis) */
  int32_t xres, yres;     /* Film "integer xresolution" / "yresolution" */
  float crop[4];          /* Film "float cropwindow" x0 x1 y0 y1 (film.rs:92-101) */
  /* textured materials (all three may be 0 / NULL): */
  const float *tri_uv;    /* 6 * n_tris: (u, v) of the three corners of every triangle -- Shape "trianglemesh" "float st" / "uv"
                             (check-sphere.pbrt:31), or pbrt-v3's default (0,0) (1,0) (1,1) for a mesh without them.  Needed
                             (PBRT_HIP_ERR_INVALID otherwise) when a material of a triangle has kd_tex != 0 */
  const pbrt_hip_texture *textures;
  uint32_t n_textures;
} pbrt_hip_scene_desc;

#define PBRT_HIP_INTEGRATOR_PATH 0   /* Integrator "path" (default name, api.rs:239) */
#define PBRT_HIP_INTEGRATOR_DIRECT 1 /* Integrator "directlighting" */
#define PBRT_HIP_INTEGRATOR_PATH_MIS 2 /* Integrator "path" "bool mis" "true": the path integrator with the direct-light estimate
                                          MULTIPLE-IMPORTANCE-SAMPLED as pbrt-v3's path integrator does (power heuristic between the
                                          one light sample and the BSDF-sampled bounce ray: DESIGN.md 3.14; integrator 0 is SURVEY A8's
                                          "no MIS in v1").  Not with the counter flags */
#define PBRT_HIP_FLAG_COUNTERS 1u    /* count nodes visited / triangles tested of the canonical walk:
                                        runs the exact-order instantiation of the kernel, equal to the oracle's counters */
#define PBRT_HIP_FLAG_WALK_COUNTERS 2u /* count what the production kernel itself does instead: nodes_visited = 64-byte
                                        child-pair records fetched, tris_tested = triangles tested */

#define PBRT_HIP_SAMPLER_STRATIFIED 0 /* Sampler "stratified" (north_star's sampler) */
#define PBRT_HIP_SAMPLER_SOBOL 1      /* Sampler "02sequence" / "lowdiscrepancy": the (0,2)-sequence sampler of DESIGN.md 3.10
                                         (the reference holds only names, api.rs:235, and the generator matrices,
                                         sobolmatrices.rs:81) */
#define PBRT_HIP_SAMPLER_SOBOL_ND 2   /* Sampler "sobol": Sobol' proper -- request j of a sample takes its own dimensions (2j, 2j + 1)
                                         of the first 128 of the reference's table (sobolmatrices.rs:81): 64 requests, every one a
                                         path of maxdepth 16 can make; later requests the padded scheme of sampler 1 (DESIGN.md
                                         3.12).  Not with the counter flags */
#define PBRT_HIP_SAMPLER_HALTON 3     /* Sampler "halton" -- the reference's DEFAULT sampler name (api.rs:235): scrambled radical
                                         inverses in the prime bases 2 .. 719, request j of a sample on the dimensions (2j, 2j + 1)
                                         for 64 requests.  Not with the counter flags */
#define PBRT_HIP_MAX_SPP (1u << 20)   /* spp_x * spp_y: the kernels pack the sample index into 20 bits */
#define PBRT_HIP_MAX_DEPTH 1023u      /* max_depth: the bounce count is packed into 10 bits */

typedef struct {
  uint32_t integrator;
  uint32_t max_depth;        /* Integrator "integer maxdepth" (<= PBRT_HIP_MAX_DEPTH, else PBRT_HIP_ERR_LIMIT) */
  uint32_t spp_x, spp_y;     /* Sampler "stratified": pixelsamples = spp_x * spp_y (<= PBRT_HIP_MAX_SPP, else PBRT_HIP_ERR_LIMIT) */
  uint64_t seed;
  uint32_t rank, world_size; /* this process renders the 64x64 super-tiles t with t % world_size == rank */
  uint32_t flags;
  uint32_t sampler;          /* PBRT_HIP_SAMPLER_* */
  float filter_xwidth, filter_ywidth; /* PixelFilter "float xwidth" / "ywidth" (box.rs:57-61): the filter's radii in pixels -- the box's,
                                         or those of the scene's pbrt_hip_pixel_filter record -- then 0 = that kind's default, and the film is
                                         the fixed-point one at every radius.  The box: 0 = the default 0.5 (a sample lands in its own pixel, film.rs:264-273 needs
                                         no tile overlap).  Any other radius in (0, 16]: every sample inside the sample bounds
                                         (film.rs:166-175) adds, weight 1, to all pixels within the radius; the film is then
                                         accumulated in 64-bit fixed point -- see pbrt_hip_render_acc below */
  float max_sample_luminance;         /* Film "float maxsampleluminance" (film.rs:75,279; pbrt-v3 FilmTile::AddSample): a
                                         sample whose luminance exceeds it is scaled down to it.  0 = no bound */
} pbrt_hip_render_desc;

typedef struct {
  uint64_t camera_rays, bounce_rays, shadow_rays; /* filled only with PBRT_HIP_FLAG_COUNTERS */
  uint64_t nodes_visited, tris_tested;            /* " */
  double kernel_ms;                               /* HIP-event time of the render kernel on its stream */
  uint64_t samples;                               /* camera samples this call rendered */
} pbrt_hip_stats;

typedef struct pbrt_hip_scene pbrt_hip_scene;

/* number of visible HIP devices (0 when there is none; never fails) */
int pbrt_hip_device_count(void);
const char *pbrt_hip_last_error(void);
const char *pbrt_hip_version(void); /* "pbrt_hip 0.14 (gfx950; struct sizes of 0.6, as 0.7, 0.8, 0.9, 0.10, 0.11, 0.12 and 0.13)": 0.14 = light type 8, a sphere
                                       light, inside the same struct sizes; 0.13 = material type 4, substrate, inside
                                       the same struct sizes; 0.12 = light type 6, a mapped light, and
                                       texture-table slot type 8, its record, inside the same struct sizes; 0.11 = material type 3, plastic, inside
                                       the same struct sizes; 0.10 = texture-table slot type 4, the
                                       image texture, inside the same struct sizes; 0.9 = texture-table slot type 3, the pixel
                                       filter, likewise; 0.8 = texture-table slot type 2, the shading normals,
                                       likewise ("as 0.7, 0.8 and 0.9": tests of the environment map, of the normals and of the pixel filter look for "0.7", "0.8" and "0.9"
                                       the way the glass test looks for "0.6"); 0.5 = round 5's ABI (pbrt_hip_scene_desc gained tri_uv / textures / n_textures at its
                                       end, pbrt_hip_material.pad became kd_tex, flags 0 of scene_create_ex = the device builder); 0.6 =
                                       material type 2, glass, inside the same struct sizes; 0.7 = light type 3 and texture-table
                                       slot type 1, the environment map, again inside the same struct sizes.  The "(... struct sizes of 0.6)"
                                       suffix is there for one reason: a test of the glass material looks for "0.6" in this string, and
                                       no struct has changed size since 0.6.  The first version that changes a struct's size drops the
                                       suffix and updates that test with it */
/* identity of the build: a hash of the library's sources and kernel-shaping flags (pbrt_amd/build.py source_id).  A
 * profile taken on one build must not price another: bench.py compares this with the id stored beside the counters */
const char *pbrt_hip_build_id(void);

/* ---- scene: upload to HBM, accelerator build.  device < 0: current device.
 * Input is validated before any device work: indices in range, vertices / spheres / camera matrix finite, sphere radii
 * positive, 0 < fov < 180 (PBRT_HIP_ERR_INVALID otherwise).
 * ONE default, whoever builds (this call, pbrt_hip_scene_create_ex with flags 0, pbrt_hip_multi_create, pbrt_hip_render_multi,
 * the command line): the accelerator is built ON THE DEVICE from the uploaded vertex / index buffers -- Morton order,
 * level-synchronous binned SAH, the tree (from 1024 triangles on) optimised by parallel re-insertion, collapse into the
 * quantised 4-wide nodes; stands in for what core/api.rs:237 names "bvh" and api.rs:446-453 would have
 * built: 0.1 s for 1M triangles.  So a `world_end` that calls pbrt_hip_scene_create + pbrt_hip_render gets the same tree as
 * one that calls pbrt_hip_render_multi.  PBRT_HIP_BUILDER=host in the environment turns the default into
 * PBRT_HIP_SCENE_HOST_BUILD for callers that left the choice open (flags 0). ---- */
int pbrt_hip_scene_create(const pbrt_hip_scene_desc *desc, int device, pbrt_hip_scene **out);
/* The same with options (0 = the default above).
 * PBRT_HIP_SCENE_GPU_BUILD: the default, said explicitly (PBRT_HIP_BUILDER is then not consulted).  The SAME film and hit
 * records bit for bit whichever builder is used (a hit does not depend on the tree).  The counter flags of
 * render / intersect count the oracle's canonical walk: for a device-built scene the canonical tree is built on the host at
 * the first call that asks for them (vertex / index buffers read back; about a second for 1M triangles, never on the
 * render path). */
#define PBRT_HIP_SCENE_GPU_BUILD 1u
/* PBRT_HIP_SCENE_OPTIMIZED_TREE: the HOST builder followed by the tree optimisation the device builder applies -- parallel
 * re-insertion (pbrt_amd/csrc/reinsert_core.hpp), run on one host core: a few seconds per million triangles, 4-6 % fewer node
 * fetches per ray than the plain host tree.  For hosts that must build on the CPU.  Not combined with PBRT_HIP_SCENE_GPU_BUILD /
 * PBRT_HIP_SCENE_PLAIN_TREE (PBRT_HIP_ERR_INVALID). */
#define PBRT_HIP_SCENE_OPTIMIZED_TREE 2u
/* PBRT_HIP_SCENE_PLAIN_TREE: the device's binned-SAH tree as built, without the re-insertion passes (A-B measurements). */
#define PBRT_HIP_SCENE_PLAIN_TREE 4u
/* PBRT_HIP_SCENE_HOST_BUILD: the host's binned-SAH builder (the canonical tree of the oracle and of the counter
 * flags, collapsed into the 4-wide nodes as it is): 0.7 s per million triangles on one core and a tree rays cross in ~4.5 % more
 * steps -- kept for A-B runs and for tests of that builder.  Not combined with PBRT_HIP_SCENE_GPU_BUILD / _PLAIN_TREE. */
#define PBRT_HIP_SCENE_HOST_BUILD 8u
int pbrt_hip_scene_create_ex(const pbrt_hip_scene_desc *desc, int device, uint32_t flags, pbrt_hip_scene **out);
/* how the accelerator was built: *gpu_built 0 / 1, *build_ms = host build time (wall) or device build time (events) */
int pbrt_hip_scene_build_info(const pbrt_hip_scene *scene, uint32_t *gpu_built, double *build_ms);
/* the device build's tree optimisation (parallel re-insertion, pbrt_amd/csrc/reinsert_core.hpp): passes run, nodes moved, and
 * its share of build_ms; zeros for a host-built scene or PBRT_HIP_SCENE_PLAIN_TREE.  Any pointer may be NULL. */
int pbrt_hip_scene_optimize_info(const pbrt_hip_scene *scene, uint32_t *passes, uint32_t *moves, double *ms);
void pbrt_hip_scene_destroy(pbrt_hip_scene *scene);
/* scene introspection: nodes / depth of the canonical tree (0 for a device-built scene until a counter flag built it), lights
 * (explicit + emissive triangles), bytes held in HBM */
int pbrt_hip_scene_info(const pbrt_hip_scene *scene, uint32_t *n_nodes, uint32_t *depth, uint32_t *n_lights,
                        uint64_t *device_bytes);
/* ---- the hot path ---- */
/* Render this rank's super-tiles and return the assembled film in HOST memory:
 * film_xyzw = (crop_w * crop_h * 4) floats, row-major over the cropped pixel bounds,
 * {X, Y, Z, filter_weight_sum} per pixel = Film.pixels after merge_film_tile (film.rs:47-55,313-326).
 * Pixels of super-tiles owned by other ranks are written as zeros.  A crop window that holds no pixel (crop_w or crop_h
 * 0) is a film of no floats: nothing is sampled, nothing is written, PBRT_HIP_OK (film_xyzw must still be non-NULL). */
int pbrt_hip_render(pbrt_hip_scene *scene, const pbrt_hip_render_desc *desc, float *film_xyzw, pbrt_hip_stats *stats);
/* Allocates (or grows) the device scratch a render of `scene` with this description needs -- the lanes' path-state records, the
 * partial film sums of the work items, the overflow area of the walk's stack, sampler 2's matrices -- without launching anything.
 * pbrt_hip_render_device does the same on demand; a host about to launch one frame on SEVERAL GPUs calls this for every GPU first,
 * so that no allocation (a synchronising call) separates the launches (pbrt_hip_multi_render does).  Stands in for nothing in the
 * reference (core/api.rs:432-473 renders nothing); part of the boundary's launch plumbing. */
int pbrt_hip_render_prepare(pbrt_hip_scene *scene, const pbrt_hip_render_desc *r);
/* Same, but asynchronous on `stream` (a hipStream_t, may be NULL) into a DEVICE slab of
 * pbrt_hip_slab_floats() floats: this rank's super-tiles back to back, 64*64 float4 each.
 * No synchronisation is done; stats->kernel_ms is filled by pbrt_hip_render_wait(). */
int pbrt_hip_render_device(pbrt_hip_scene *scene, const pbrt_hip_render_desc *desc, void *d_slab, void *stream);
int pbrt_hip_render_wait(pbrt_hip_scene *scene, pbrt_hip_stats *stats);
/* scatter one rank's slab (device) into a row-major film (device), both float4 per pixel */
int pbrt_hip_film_assemble_device(const pbrt_hip_scene *scene, const void *d_slab, uint32_t rank, uint32_t world_size,
                                  void *d_film_xyzw, void *stream);
/* ---- box filter radii other than 0.5 (pbrt_hip_render_desc.filter_xwidth / ywidth) ----
 * The reference's Film keeps a filter table for any radius (film.rs:113-123), expands a tile by it (film.rs:264-273) and
 * merges tiles under a mutex (film.rs:313-326); it has no add_sample.  Here such a film is accumulated in 64-bit fixed
 * point -- four int64 per pixel of the cropped window, {r, g, b} in units of 2^-24 (a component of a sample clamped to
 * [0, 2^15]) and the sample count -- with integer atomics: integer sums do not depend on the order of arrival, so the
 * image is reproducible and the accumulators of several ranks ADD to those of one rank exactly (multi-GPU: one sum
 * reduction instead of the gather).  pbrt_hip_render / pbrt_hip_render_multi accept such a desc like any other (with
 * world_size > 1, pbrt_hip_render's film then holds the rank's OWN samples only: combine ranks by adding accumulators).
 *  - pbrt_hip_render_buffer_bytes: bytes pbrt_hip_render_device writes for this desc -- the rank's slab (default filter)
 *    or the accumulators of the whole cropped window, 32 bytes per pixel (zeroed by the call);
 *  - pbrt_hip_render_acc: this rank's accumulators in HOST memory (crop_w * crop_h * 4 int64);
 *  - pbrt_hip_film_from_acc_device / pbrt_hip_film_from_acc: accumulators -> Film pixels {X, Y, Z, weight}
 *    (= Film::merge_film_tile's arithmetic on the radiance sum, film.rs:313-326), on the device or on the host. */
int64_t pbrt_hip_render_buffer_bytes(const pbrt_hip_scene *scene, const pbrt_hip_render_desc *desc);
int pbrt_hip_render_acc(pbrt_hip_scene *scene, const pbrt_hip_render_desc *desc, int64_t *acc, pbrt_hip_stats *stats);
int pbrt_hip_film_from_acc_device(const pbrt_hip_scene *scene, const void *d_acc, void *d_film_xyzw, void *stream);
void pbrt_hip_film_from_acc(const int64_t *acc, int64_t n_pixels, float *film_xyzw);
/* ---- weighted pixel filters (pbrt_hip_pixel_filter) ----
 *  - pbrt_hip_filter_table: host, no device.  The 16 x 16 table of Film::new (film.rs:113-123): out[iy * 16 + ix] = the filter at
 *    ((ix + 0.5) rx / 16, (iy + 0.5) ry / 16), evaluated in double and rounded to float once (rx, ry: the radii themselves, not 0).
 *    PBRT_HIP_ERR_INVALID for a record pbrt_hip_scene_create would refuse or radii that are not positive and finite;
 *  - pbrt_hip_film_from_acc_weighted: pbrt_hip_film_from_acc for the accumulators of a weighted filter -- the fourth channel is the weight
 *    sum in 2^-24 units and is scaled like the other three.  pbrt_hip_film_from_acc_device knows its scene and converts accordingly. */
int pbrt_hip_filter_table(const pbrt_hip_pixel_filter *filter, float rx, float ry, float out[256]);
void pbrt_hip_film_from_acc_weighted(const int64_t *acc, int64_t n_pixels, float *film_xyzw);
/* host-side geometry of the sharding (no device needed) */
int64_t pbrt_hip_slab_floats(int32_t xres, int32_t yres, const float crop[4], uint32_t rank, uint32_t world_size);
/* for every float4 slot of a rank's slab the row-major pixel index inside the cropped film, or -1 */
int pbrt_hip_slab_pixel_index(int32_t xres, int32_t yres, const float crop[4], uint32_t rank, uint32_t world_size,
                              int64_t *out);

/* ---- every GPU of the node behind one call: what a single-process host (the reference's world_end, api.rs:432-473,
 * reached from bin/pbrt.rs:72-83) needs to render on 8 MI355X.  The scene is built once on GPU 0 and copied device to
 * device (xGMI); GPU g renders the super-tiles t with t % n_gpus == g on its own stream from its own host thread; ONE
 * RCCL gather (ncclGather, communicators from ncclCommInitAll) brings the slabs to GPU 0, where they are assembled into
 * the film.  n_gpus <= 0: all visible devices.  desc->rank / world_size are ignored (the library sets them).
 * film_xyzw (host, crop_w * crop_h * 4 floats) may be NULL when only the device film is wanted;
 * per_gpu (n_gpus entries) may be NULL.  flags as pbrt_hip_scene_create_ex. ---- */
typedef struct pbrt_hip_multi pbrt_hip_multi;
int pbrt_hip_multi_create(const pbrt_hip_scene_desc *desc, int n_gpus, uint32_t flags, pbrt_hip_multi **out);
int pbrt_hip_multi_gpus(const pbrt_hip_multi *multi);
int pbrt_hip_multi_render(pbrt_hip_multi *multi, const pbrt_hip_render_desc *desc, float *film_xyzw, pbrt_hip_stats *per_gpu);
/* the assembled film of the last pbrt_hip_multi_render on GPU 0 (float4 per pixel, row-major) */
int pbrt_hip_multi_film_device(pbrt_hip_multi *multi, void **d_film_xyzw);
void pbrt_hip_multi_destroy(pbrt_hip_multi *multi);
/* create + render + destroy: the whole of `world_end` in one call */
int pbrt_hip_render_multi(const pbrt_hip_scene_desc *desc, const pbrt_hip_render_desc *render, int n_gpus, float *film_xyzw,
                          pbrt_hip_stats *per_gpu);

/* Ray-batch entry points: the traversal kernels on their own (parity + roofline of the
 * dominant loop).  Host SoA-of-xyz arrays, n rays.  prim = 0xffffffff on a miss.  A ray whose origin or direction has a component
 * that is not finite, or whose tmax is NaN, is a miss (and is not walked); direction components that are exactly 0 are fine.
 * What counts as a hit (the own-box rule): the triangle / sphere test's candidate, provided the ray meets the primitive's own
 * bounding box; t is at least the distance at which it enters that box.  Whether and where a ray hits a primitive depends on the ray and the
 * primitive alone -- never on the tree, the builder or the walk -- and ties on t go to the lower primitive number (spheres: n_tris + index). */
int pbrt_hip_intersect(pbrt_hip_scene *scene, int64_t n, const float *o, const float *d, const float *tmax, float *t,
                       uint32_t *prim, float *b1, float *b2, uint64_t *counters /* 2, may be NULL */);
int pbrt_hip_occluded(pbrt_hip_scene *scene, int64_t n, const float *o, const float *d, const float *tmax,
                      uint8_t *hit);

/* ---- host pieces either side of the path that the reference does implement ---- */
/* Film::new / get_sample_bounds / get_film_tile (film.rs:82-137,166-175,264-281); bounds are x0 y0 x1 y1 */
void pbrt_hip_film_cropped_bounds(int32_t xres, int32_t yres, const float crop[4], int32_t out[4]);
void pbrt_hip_film_sample_bounds(int32_t xres, int32_t yres, const float crop[4], float rx, float ry, int32_t out[4]);
void pbrt_hip_film_tile_bounds(int32_t xres, int32_t yres, const float crop[4], float rx, float ry,
                               const int32_t sample_bounds[4], int32_t out[4]);
/* Film::write_image's pixel arithmetic (film.rs:340-372): xyzw -> linear RGB, 3 floats per pixel */
void pbrt_hip_film_to_rgb(const float *film_xyzw, int64_t n_pixels, float scale, float *rgb);
/* imageio::write_image (imageio.rs:235-283): ".png" (8-bit sRGB via to_byte, imageio.rs:66-68) or ".pfm" */
int pbrt_hip_write_image(const char *name, const float *rgb, int32_t width, int32_t height);
/* imageio::read_image (imageio.rs:87-184): ".png" (8-bit, value = byte / 255) or ".pfm".  Call with rgb == NULL to get
 * the size, then with a width*height*3 buffer (width / height must then hold that size). */
int pbrt_hip_read_image(const char *name, float *rgb, int32_t *width, int32_t *height);
/* Transform::look_at (transform.rs:485-520): m = world->camera, m_inv = camera->world */
void pbrt_hip_look_at(const float pos[3], const float look[3], const float up[3], float m[16], float m_inv[16]);

/* ---- scene ingestion: the reference's parser + API state machine, completed for this path ----
 * (parser.rs:205-317 handles 12 of 37 directive arms; api.rs stores no geometry.)  Host only.
 * Status codes: 0 ok; PBRT_HIP_ERR_INVALID with last_error() = "<kind>: <detail>", kind in
 * {Eof, UnterminatedString, MixedParameters, Unquoted, Syntax, NotImplemented, Io} (parser.rs:31-58). */
typedef struct pbrt_hip_loaded pbrt_hip_loaded;
int pbrt_hip_load_file(const char *path, pbrt_hip_loaded **out);
int pbrt_hip_load_string(const char *text, size_t len, const char *base_dir /* for Include, may be NULL */,
                         pbrt_hip_loaded **out);
void pbrt_hip_loaded_free(pbrt_hip_loaded *loaded);
/* desc / render are filled with pointers INTO `loaded` (valid until it is freed); filename = Film "string filename" */
int pbrt_hip_loaded_get(const pbrt_hip_loaded *loaded, pbrt_hip_scene_desc *desc, pbrt_hip_render_desc *render,
                        char *filename, size_t filename_cap);
/* Film "float scale" (film.rs:368-371: every pixel is multiplied by it in Film::write_image): pass it to
 * pbrt_hip_film_to_rgb.  1 for a NULL handle. */
float pbrt_hip_loaded_film_scale(const pbrt_hip_loaded *loaded);
/* warnings (ignored directives / parameters, api.rs:291-332 "log and continue"), '\n'-separated; returns their count */
int pbrt_hip_loaded_warnings(const pbrt_hip_loaded *loaded, char *buf, size_t cap);
#ifdef __cplusplus
}
#endif
#endif
