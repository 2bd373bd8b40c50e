// tri_test.inc -- the triangle test of the walk's leaf pass, stated once as text: included by trav_run (kernel_walk.hpp) and by the
// building-blocks kernel (kernels_blocks.hip: op TRI_HIT), so that the tests of tests/test_blocks_*.py run the statements the render
// kernels run.  (Text and not a function: every function form tried changed the render kernels' machine code.)  Reads the locals
//   float4 a, b, c   the triangle's record: xyz = p0, p1, p2        V3 o, d, inv1   the ray and its TRUE 1 / d        T.tmax
// and leaves  bool valid;  float tsnap (the hit's distance: max(th, the own box's entry)), u, v  behind.
// Moeller-Trumbore, operation order of DESIGN.md 3.5
const V3 p0 = xyz(a);
const V3 e1 = xyz(b) - p0, e2 = xyz(c) - p0;
const V3 pv = cross(d, e2);
const float det = dot(e1, pv);
// Branch-free from here: every lane of the pass computes u, v and t (a degenerate triangle's 1 / det is inf or
// NaN and fails the tests below like any miss) and the hit record is updated by selects.  The nested early-outs
// this replaces skipped work only when ALL lanes of the pass failed the same test, and the compiler paid for
// them with copies of the six hit-record registers at every level (about 50 v_mov per pass).
const float idet = 1.0f / det;
const V3 tv = o - p0;
const float u = dot(tv, pv) * idet;
const V3 qv = cross(tv, e1);
const float v = dot(d, qv) * idet;
const float th = dot(e2, qv) * idet;
// The own-box rule (DESIGN.md 3.5; round 6): the ray must MEET the triangle's own box -- the node test of 3.4 on it: slab distances
// of the three vertices with the TRUE 1 / d (two roundings each, as the canonical node test; p0 - o = -tv exactly), their min / max
// per axis, pad kOwnPad < kBoxPad -- and the hit's distance is at least the box's entry: t = max(th, entry).  Monotone arithmetic:
// every enclosing box of every tree then passes its own test while the walk's best hit is still >= t, so an accepted hit is reached
// by every walk and a hit is a function of (ray, triangle) alone.  (Raising t instead of rejecting: a triangle flat in an axis plane
// has entry = exit = the plane's slab distance, which Moeller-Trumbore's t misses by rounding.)
#ifdef PBRT_NO_OWN_BOX_RULE  // A-B switch: the leaf pass as it was until round 5 (what the rule costs; films differ where it rejects)
const bool in_own_box = true;
const float tsnap = th;
#else
const V3 w1 = xyz(b) - o, w2 = xyz(c) - o;
const float x0 = (-tv.x) * inv1.x, x1 = w1.x * inv1.x, x2 = w2.x * inv1.x;
const float y0 = (-tv.y) * inv1.y, y1 = w1.y * inv1.y, y2 = w2.y * inv1.y;
const float z0 = (-tv.z) * inv1.z, z1 = w1.z * inv1.z, z2 = w2.z * inv1.z;
const float otn = fmaxf(fmaxf(fminf(fminf(x0, x1), x2), fminf(fminf(y0, y1), y2)), fmaxf(fminf(fminf(z0, z1), z2), kRayTMin));
const float otf = fminf(fminf(fmaxf(fmaxf(x0, x1), x2), fmaxf(fmaxf(y0, y1), y2)), fmaxf(fmaxf(z0, z1), z2));
const bool in_own_box = otn <= otf * kOwnPad;
const float tsnap = fmaxf(th, otn);
#endif
bool valid = in_own_box && !(fabsf(det) < 1e-8f) && (u >= 0.f) && (v >= 0.f) && (u + v <= 1.0f) && (th > kRayTMin) && (tsnap < T.tmax);
