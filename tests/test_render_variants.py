"""pbrt_amd/csrc/render_variant.hpp -- the one statement of which render-kernel variants exist, which family renders them and with which
register budget -- against the rules restated here, against the kernels of the built library, and against the stack plan.  No GPU."""
import collections
import ctypes as C
import itertools

from pbrt_amd import _lib, isa_id
import render_variant_table as rvt
from render_variant_table import COUNT_EXACT, COUNT_NONE, COUNT_WALK

INVALID, LIMIT = -1, -4  # PBRT_HIP_ERR_INVALID, PBRT_HIP_ERR_LIMIT


# ---- the rules, restated: check_render_desc's refusals in its order, launch_render's order of questions, the kernels' launch bounds ----

def refusal(v):
    """(code, a word of the message) or (0, None)"""
    counting = v.counters != COUNT_NONE
    if v.table_sampler and counting: return INVALID, "Sobol' / Halton"
    if v.wide and counting: return INVALID, "box filter"
    if v.normals and counting: return LIMIT, "normals"
    if v.normals and v.wide: return LIMIT, "normals"
    if v.env and counting: return LIMIT, "environment map"
    if (v.textured or v.mis) and counting: return LIMIT, "textured materials / the MIS integrator"
    if v.glass and counting: return LIMIT, "glass"
    if v.env and v.wide: return LIMIT, "environment map"
    return 0, None


def family(v):
    if v.normals: return "n"
    if v.env: return "env"
    if v.counters == COUNT_EXACT: return "default"
    if v.glass or v.mis or v.textured or (v.table_sampler and v.wide): return "x"
    return "default"


def default_path(v):
    return family(v) == "default" and v.counters == COUNT_NONE and not v.wide and not v.table_sampler


def budget(v):
    return {"n": 4, "env": 4}.get(family(v), 3 if v.spheres or v.glass else 5)


def test_table_is_the_rules():
    """Every one of the 768 variants: the header compiles without HIP, refuses what check_render_desc refused with its code and message, and
    sends what it accepts to the family launch_render sent it to, with that family's launch bounds."""
    rows = rvt.table()
    assert len(rows) == 768 and len({r[:9] for r in rows}) == 768
    for r in rows:
        code, word = refusal(r)
        assert r.code == code, r
        if code:
            assert word in r.text and r.text.startswith("render: "), r
            continue
        assert r.text == "" and r.family == family(r) and r.default_path == default_path(r) and r.waves_per_simd == budget(r), r
    assert collections.Counter(r.family if r.code == 0 else "refused" for r in rows) == {"refused": 604, "default": 10, "x": 58, "env": 32, "n": 64}
    # the messages the GPU refusal tests match on, with the codes they expect
    said = {(r.code, w) for r in rows for w in ("normals", "environment map", "box filter", "glass") if r.code and w in r.text}
    assert said == {(LIMIT, "normals"), (LIMIT, "environment map"), (INVALID, "box filter"), (LIMIT, "box filter"), (LIMIT, "glass")}
    # a refusal never depends on the spheres (rows i and i ^ 1 differ in that switch alone)
    assert all(r.code == rows[i ^ 1].code and r.spheres != rows[i ^ 1].spheres for i, r in enumerate(rows))


# ---- the kernels of the library: exactly what the accepted variants reach ----

NAMES = {
    "default": "render_kernel<{spheres},{count},{exact},{stack},{steps},{wide},{table_sampler}>",
    "x": "render_kernel_x<{spheres},{stack},{mis},{textured},{table_sampler},{wide},{glass}>",
    "env": "render_kernel_env<{spheres},{stack},{mis},{textured},{table_sampler}>",  # (GLS is folded away: always true)
    "n": "render_kernel_n<{spheres},{stack},{mis},{textured},{table_sampler},{env}>",  # (likewise)
}
STACK_OVERFLOW, STEPS, EXACT_ROWS = 30, 3, (20, 26, 32, 40, 64)


def kernel_names(r):
    """the instantiations a launch of accepted variant `r` may run, whatever the tree"""
    sw = {k: str(getattr(r, k)).lower() for k in rvt.SWITCHES}
    sw.update(count=str(r.counters != COUNT_NONE).lower(), exact=str(r.counters == COUNT_EXACT).lower(), steps=STEPS)
    if r.counters == COUNT_EXACT:
        return {NAMES[r.family].format(**sw, stack=rows_) for rows_ in EXACT_ROWS}
    names = {NAMES[r.family].format(**sw, stack=stack) for stack in (0, STACK_OVERFLOW)}
    if r.default_path:
        names.add(NAMES[r.family].format(**{**sw, "steps": 2}, stack=0))  # shallow trees: 2 node steps per check
    return names


def test_library_holds_exactly_the_reachable_kernels():
    """The set of render-kernel instantiations is derived from the table (the launchers' `if constexpr`): every kernel an accepted variant
    can launch is in the library, and the library holds no render kernel that no render description reaches."""
    reachable = set().union(*(kernel_names(r) for r in rvt.table() if r.code == 0))
    built = {isa_id.normalise(k) for k in isa_id.kernel_ids(_lib.LIB_PATH)}
    built = {k for k in built if k.startswith("render_kernel")}
    assert reachable == built, (sorted(reachable - built), sorted(built - reachable))
    assert len(built) == 240
    assert collections.Counter(k.split("<")[0] for k in built) == {"render_kernel": 28, "render_kernel_x": 116, "render_kernel_env": 32, "render_kernel_n": 64}


# ---- the grid: waves per CU = what the registers and the stack plan's LDS both allow ----

def plan_waves(need, default_path_launch):
    u = [C.c_uint32() for _ in range(4)]
    if default_path_launch:
        assert _lib.lib().pbrt_hip_render_stack_layout(need, *map(C.byref, u)) == 0
        return u[2].value
    assert _lib.lib().pbrt_hip_render_stack_plan(need, *map(C.byref, u[:3])) == 0
    return u[1].value


def test_waves_per_cu_follow_budget_and_plan():
    for need, dflt in itertools.product((6, 16, 28, 29, 44), (False, True)):
        waves = plan_waves(need, dflt)
        assert waves == 20, (need, dflt, waves)  # (30 rows or fewer, records included: tests/test_host.py, tests/test_lds_path_records.py)
        seen = set()
        for r in rvt.table(waves):
            if r.code or r.default_path != dflt:
                continue
            assert r.waves_per_cu == min(4 * r.waves_per_simd, waves), (need, r)
            kind = r.family if r.family in ("env", "n") else ("spheres / glass" if r.spheres or r.glass else "plain")
            seen.add((kind, r.waves_per_cu))
        assert seen == ({("plain", 20), ("spheres / glass", 12)} | (set() if dflt else {("env", 16), ("n", 16)})), (need, dflt, seen)
    # a plan with fewer waves than the registers allow wins
    assert {r.waves_per_cu for r in rvt.table(10) if r.code == 0} == {10}
    assert {(r.family, r.waves_per_cu) for r in rvt.table(14) if r.code == 0 and not (r.spheres or r.glass)} == {("default", 14), ("x", 14), ("env", 14), ("n", 14)}
