// quad_nearest.inc -- the child a node step enters, stated once as text: included by trav_run (kernel_walk.hpp) after quad_step and by
// the building-blocks kernel (kernels_blocks.hip: ops QUAD_STEP*).  (Text and not a function, as tri_test.inc: the function forms tried
// -- flags by reference, written at the end, returned as a struct -- changed the render kernels' machine code.)  Reads and overwrites
// float key[4] (a missed child's key becomes NaN), reads bool hit[4]; leaves bool n0 .. n3 behind: the hit child of least entry distance,
// the lowest slot on a tie, n3 = none of the first three.
#pragma unroll
// (a missed child's key is a NaN with all bits set -- an inline constant of the select, where +inf would need a
// register; fminf ignores it, and when every child is missed nothing below uses kmin)
for (int k = 0; k < 4; k++) key[k] = hit[k] ? key[k] : __uint_as_float(0xffffffffu);
const float kmin = fminf(fminf(key[0], key[1]), fminf(key[2], key[3]));
const bool n0 = key[0] == kmin, n1 = !n0 && key[1] == kmin, n2 = !n0 && !n1 && key[2] == kmin;
const bool n3 = !n0 && !n1 && !n2;
