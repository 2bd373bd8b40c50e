"""pbrt_amd/csrc/render_variant.hpp as a table: a stand-alone program (plain g++, no HIP) prints, for each of the 2^8 x 3 variants, what the
header says of it.  Compiled once per session; tests/test_render_variants.py holds the table to the rules, and the register-budget tests of
the kernel families take their waves per SIMD from it."""
import atexit
import collections
import functools
import os
import shutil
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SWITCHES = ("spheres", "wide", "table_sampler", "mis", "textured", "glass", "env", "normals")  # RenderVariant's order
FAMILIES = ("default", "x", "env", "n")  # RenderFamily's order
COUNT_NONE, COUNT_EXACT, COUNT_WALK = 0, 1, 2
Row = collections.namedtuple("Row", SWITCHES + ("counters", "code", "text", "family", "default_path", "waves_per_simd", "waves_per_cu"))

PROGRAM = r"""
#include <stdio.h>
#include <stdlib.h>
#include "render_variant.hpp"
using namespace pbrt_hip;
static_assert(render_family_builds(RenderFamily::kDefault, RenderVariant{}), "the table is usable in constant expressions");
int main(int argc, char **argv) {
  const uint32_t plan_waves = argc > 1 ? (uint32_t)atoi(argv[1]) : 0u;
  for (int c = 0; c < 3; c++)
    for (int m = 0; m < 256; m++) {
      const RenderVariant v{(m & 1) != 0, (m & 2) != 0, (m & 4) != 0, (m & 8) != 0, (m & 16) != 0, (m & 32) != 0, (m & 64) != 0, (m & 128) != 0, (RenderCounters)c};
      const RenderRefusal no = render_variant_refusal(v);
      const RenderFamily f = render_family(v);
      printf("%d %d %d %d %d %u %u|%s\n", m, c, no.code, (int)f, (int)render_default_path(v), render_waves_per_simd(f, v.spheres, v.glass),
             render_waves_per_cu(v, plan_waves), no.text ? no.text : "");
    }
  return 0;
}
"""


@functools.lru_cache(maxsize=None)
def _program():
    d = tempfile.mkdtemp(prefix="render_variants_")
    atexit.register(shutil.rmtree, d, ignore_errors=True)
    src, exe = os.path.join(d, "dump.cpp"), os.path.join(d, "dump")
    with open(src, "w") as f:
        f.write(PROGRAM)
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "pbrt_amd", "csrc"), src, "-o", exe], check=True)
    return exe


@functools.lru_cache(maxsize=None)
def table(plan_waves=20):
    """the 768 rows; waves_per_cu is the header's answer for a stack plan of `plan_waves` waves per CU"""
    rows = []
    for line in subprocess.run([_program(), str(plan_waves)], check=True, capture_output=True, text=True).stdout.splitlines():
        nums, text = line.split("|", 1)
        m, c, code, fam, dflt, wps, wpc = (int(x) for x in nums.split())
        rows.append(Row(*[bool(m >> k & 1) for k in range(8)], c, code, text, FAMILIES[fam], bool(dflt), wps, wpc))
    return tuple(rows)


def waves_per_simd(family, **switches):
    """the one register budget of the accepted variants of `family` whose switches are as given"""
    found = {r.waves_per_simd for r in table() if r.code == 0 and r.family == family and all(getattr(r, k) == v for k, v in switches.items())}
    assert len(found) == 1, (family, switches, found)
    return found.pop()
