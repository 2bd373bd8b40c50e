// leaf_test.inc -- one parked lane's triangle (or sphere) against its ray and the update of the lane's hit record, stated once as
// text: included by trav_run (kernel_walk.hpp) in the straight-line leaf pass of single-triangle leaves and in the counted loop that
// serves leaves of several triangles and the exact walk.  Reads the locals
//   uint32_t first, i   the leaf's first slot and the triangle's place in it        bool stop        tris, o, d, inv1, T, ct
// and updates T.h, T.any and stop (an any-hit ray ends at its first valid hit).
          const uint32_t slot = first + i;
          wave_prio(PBRT_PRIO_FETCH);  // (as for the node fetch)
          const float4 a = EXP_TRI_LOAD(reinterpret_cast<const float4 *>(tris + slot * (16u * kTriStride)));
          const float4 b = EXP_TRI_LOAD(reinterpret_cast<const float4 *>(tris + slot * (16u * kTriStride) + 16u));
          const float4 c = EXP_TRI_LOAD(reinterpret_cast<const float4 *>(tris + slot * (16u * kTriStride) + 32u));
          wave_prio(PBRT_PRIO_ARITH);
          if (COUNT) ct++;
#include "tri_test.inc"
          float ht = tsnap, hu = u, hv = v;
          if (SPH && __float_as_uint(c.w) != 0u) {
            // a SPHERE's record (round 6: spheres are primitives of the tree, DESIGN.md 3.5): {centre, primitive id}{radius, -, -, material}
            // {-, -, -, 1}.  Sphere::Intersect with the f64 quadratic of lib.rs:181-203, then the own-box rule on [c - r, c + r] (the
            // "vertices" lo, hi, lo) exactly as for a triangle.
            const float r = b.x;
            float ts = 0.f;
            valid = sphere_hit(make_float4(a.x, a.y, a.z, r), o, d, T.tmax, ts);
            const V3 lo = {a.x - r, a.y - r, a.z - r}, hi = {a.x + r, a.y + r, a.z + r};
            const float sx0 = (lo.x - o.x) * inv1.x, sx1 = (hi.x - o.x) * inv1.x, sy0 = (lo.y - o.y) * inv1.y, sy1 = (hi.y - o.y) * inv1.y;
            const float sz0 = (lo.z - o.z) * inv1.z, sz1 = (hi.z - o.z) * inv1.z;
            const float stn = fmaxf(fmaxf(fminf(fminf(sx0, sx1), sx0), fminf(fminf(sy0, sy1), sy0)), fmaxf(fminf(fminf(sz0, sz1), sz0), kRayTMin));
            const float stf = fminf(fminf(fmaxf(fmaxf(sx0, sx1), sx0), fmaxf(fmaxf(sy0, sy1), sy0)), fmaxf(fmaxf(sz0, sz1), sz0));
            ht = fmaxf(ts, stn);
            valid = valid && stn <= stf * kOwnPad && ht < T.tmax;
            hu = 0.f; hv = 0.f;
          }
          const uint32_t id = __float_as_uint(a.w);
          const bool occl = valid && T.any != 0u;  // any-hit ray: the walk ends at the first valid hit
          const bool closer = valid && T.any == 0u && (ht < T.h.t || (ht == T.h.t && id < T.h.prim));
          T.any = occl ? 3u : T.any;
          stop = stop || occl;
          T.h.t = closer ? ht : T.h.t;
          T.h.prim = closer ? id : T.h.prim;
          T.h.slot = closer ? slot : T.h.slot;
          T.h.b1 = closer ? hu : T.h.b1;
          T.h.b2 = closer ? hv : T.h.b2;
