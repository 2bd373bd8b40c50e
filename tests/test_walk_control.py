"""The control code of the walk (kernel_walk.hpp trav_run, round 7): the scheduling decisions are mask arithmetic on the scalar unit, the loop
is rotated, and the leaf pass of single-triangle leaves is straight-line, with the counted loop out of line.  No arithmetic statement moved, so
nothing computed may change: films, hit records and occlusion flags equal the oracle's bit for bit, the canonical counters equal the oracle's
and the production walk's equal the totals recorded before (tests/golden/lds_path_records_walk.json).  The host tests look at the machine
code of the production instantiation and at the guarantee the straight-line pass leans on: leaves of at most one triangle."""
import glob
import json
import os
import re
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

from pbrt_amd import _lib, api, scenes
from util import assert_bit_equal, random_rays

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lds_path_records_walk.json")
COUNTERS = ("camera_rays", "bounce_rays", "shadow_rays", "nodes_visited", "tris_tested")
LLVM = "/opt/rocm/lib/llvm/bin"
PRODUCTION = "_ZN8pbrt_hip12_GLOBAL__N_113render_kernelILb0ELb0ELb0ELi30ELi3ELb0ELb0EEEvNS_8DevSceneENS_12RenderParamsE"
MESH_KW = dict(max_depth=8, spp=(2, 2), seed=3)  # (the golden file's case: mesh20k_64x64_2x2_depth8_seed3_host)


# ---- host: the machine code ----

def disassembly(symbol):
    """[(byte offset in the function, mnemonic, operands, branch target's offset or None)] of a kernel of the built library"""
    with tempfile.TemporaryDirectory() as td:
        so = shutil.copy(_lib.LIB_PATH, td)
        subprocess.run([os.path.join(LLVM, "llvm-objdump"), "--offloading", os.path.basename(so)], cwd=td, check=True, capture_output=True)
        text = ""
        for co in sorted(glob.glob(os.path.join(td, "*gfx950"))):
            r = subprocess.run([os.path.join(LLVM, "llvm-objdump"), "-d", "--disassemble-symbols=" + symbol, co], capture_output=True, text=True)
            if "s_endpgm" in r.stdout:
                text = r.stdout
    assert text, "the production instantiation was not found in the library's gfx950 code objects"
    out, base = [], None
    for line in text.split("\n"):
        m = re.match(r"\s+(\w+)\s*(.*?)\s*// ([0-9A-F]{12}):", line)
        if not m:
            continue
        addr = int(m.group(3), 16)
        base = addr if base is None else base
        t = re.search(r"<[^>]*\+0x([0-9a-f]+)>\s*$", line) if m.group(1).startswith(("s_cbranch", "s_branch")) else None
        out.append((addr - base, m.group(1), m.group(2), int(t.group(1), 16) if t else None))
    return out


def load_groups(ins, widths):
    """indices at which a run of len(widths) CONSECUTIVE global loads starts whose widths (dwords), sorted by their offset: field, are `widths`"""
    found = []
    for i in range(len(ins) - len(widths) + 1):
        run = ins[i:i + len(widths)]
        if not all(r[1].startswith("global_load_dwordx") for r in run) or (i and ins[i - 1][1].startswith("global_load_dwordx")):
            continue
        if i + len(widths) < len(ins) and ins[i + len(widths)][1].startswith("global_load_dwordx"):
            continue
        offs = sorted((int((re.search(r"offset:(\d+)", r[2]) or [0, 0])[1]), int(r[1][-1])) for r in run)
        if [o for o, _ in offs] == [16 * k for k in range(len(widths))] and [w for _, w in offs] == list(widths):
            found.append(i)
    return found


def census(ins):
    valu = sum(1 for i in ins if i[1].startswith("v_"))
    salu = sum(1 for i in ins if i[1].startswith("s_"))
    return {"instructions": len(ins), "valu": valu, "salu": salu, "memory": len(ins) - valu - salu,
            "v_mov": sum(1 for i in ins if i[1].startswith("v_mov")), "v_cndmask": sum(1 for i in ins if i[1].startswith("v_cndmask"))}


@pytest.mark.skipif(not os.path.exists(os.path.join(LLVM, "llvm-objdump")), reason="needs the ROCm llvm tools")
def test_walk_loop_of_the_production_kernel():
    """The walk loop of render_kernel<false, false, false, 30, 3, false, false> as it came out: the innermost loop that holds every node fetch
    (four global_load_dwordx4 of one 64-byte node) holds exactly three of them -- STEPS = 3, no step duplicated into a side path -- and, in
    the straight-line run from its head to its backward branch, ONE triangle fetch (16 + 12 + 12 bytes of a record): the leaf pass of
    single-triangle leaves.  The counted loop for larger leaves has the only other one, out of line behind the loop.  The instruction
    counts of the loop and its parts are printed, not asserted (DESIGN.md section 6 has the figures this round started from)."""
    ins = disassembly(PRODUCTION)
    nodes = load_groups(ins, (4, 4, 4, 4))
    tris = load_groups(ins, (4, 3, 3))
    assert len(nodes) == 3, [hex(ins[i][0]) for i in nodes]
    lo, hi = ins[nodes[0]][0], ins[nodes[-1]][0]
    loops = [(t, off) for off, op, _, t in ins if t is not None and t <= lo and off >= hi]  # backward branches round all three
    assert loops, "no loop holds the three node fetches"
    head, back = max(loops)  # the innermost
    inside = [i for i in ins if head <= i[0] <= back]
    n_in = [i for i in nodes if head <= ins[i][0] <= back]
    t_in = [i for i in tris if head <= ins[i][0] <= back]
    print("walk loop %#x .. %#x:" % (head, back), census(inside))
    print("  head, up to the first node fetch:", census([i for i in inside if i[0] < lo]))
    if t_in:
        t0 = ins[t_in[0]][0]
        flush = max((i[0] for i in inside if i[0] < t0 and i[0] > hi and i[1].startswith("s_bcnt1")), default=t0)
        print("  the three node steps:", census([i for i in inside if lo <= i[0] < flush]))
        print("  leaf decision, leaf pass, pop and the loop's exit test:", census([i for i in inside if i[0] >= flush]))
    assert len(n_in) == 3
    assert len(t_in) == 1, [hex(ins[i][0]) for i in tris]
    assert len(tris) == 2 and ins[[i for i in tris if i not in t_in][0]][0] > back, [hex(ins[i][0]) for i in tris]


# ---- the guarantee of the straight-line leaf pass ----

def leaf_counts(quads):
    """the triangle counts of every leaf ref of a tree's quad nodes (words 12..15 of a node: kLeafRef | count << 24 | first slot)"""
    refs = np.asarray(quads, np.uint32).reshape(-1, 16)[:, 12:16].reshape(-1)
    leaves = refs[(refs & 0x80000000) != 0]
    return (leaves >> 24) & 0x7f


def soup():
    sd = scenes.random_mesh_scene(5_000, 32, 32)
    return sd


def test_host_built_trees_have_leaves_of_one_triangle():
    """Every leaf ref of the host builder's quantised tree of a 5 000-triangle soup holds one triangle or none (kEmptyLeafRef, an unused child
    slot): a leaf of 2 .. 4 triangles became a quad node of them (quad_nodes.cpp).  The straight-line leaf pass serves all of them; the counted
    loop behind it is for a tree built otherwise."""
    sd = soup()
    for tree in ("default", "sah", "reinsert"):
        cnt = leaf_counts(api.quad_build_host_ex(sd.P, sd.idx, tree=tree)["quads"])
        assert cnt.size > 5_000 and cnt.max() <= 1 and (cnt == 1).sum() == sd.idx.shape[0], (tree, np.bincount(cnt))


@pytest.mark.gpu
def test_trees_in_device_memory_have_leaves_of_one_triangle(gpu):
    """the same of the trees as they sit in HBM (export_quads), host-built and device-built"""
    sd = soup()
    for builder in ("host", "gpu", "gpu-plain"):
        with gpu.Scene(sd, builder=builder) as sc:
            cnt = leaf_counts(sc.export_quads()[0])
        assert cnt.size > 5_000 and cnt.max() <= 1 and (cnt == 1).sum() == sd.idx.shape[0], (builder, np.bincount(cnt))


# ---- GPU: nothing computed changed ----

@pytest.fixture(scope="module")
def mesh(oracle):
    """the 20 000-triangle mesh at 64 x 64 (on the host builder's tree: stack bound 29, the overflow variant with its records in LDS and
    STEPS = 3) and the oracle's film and counters of it, computed once"""
    sd = scenes.random_mesh_scene(20_000, 64, 64)
    film, st = oracle.OracleScene(sd).render(**MESH_KW)
    return sd, film, st


@pytest.mark.gpu
def test_mesh_film_and_counters(gpu, mesh):
    """film equal to the oracle's; counters=True -- the EXACT walk, whose leaves hold several triangles: the counted loop alone -- equal to
    the oracle's counters, its film too; counters="walk" -- the production walk counting its own fetches and tests -- equal to the totals
    recorded in tests/golden/ before the control code changed: the same nodes fetched, the same triangles tested."""
    sd, ref, rst = mesh
    with gpu.Scene(sd, builder="host") as sc:
        assert sc.info()["quad_stack_need"] > 28  # the precondition: the overflow variant
        film, _ = sc.render(**MESH_KW)
        cfilm, cst = sc.render(counters=True, **MESH_KW)
        wfilm, wk = sc.render(counters="walk", **MESH_KW)
    assert_bit_equal(film, ref, "film")
    assert_bit_equal(cfilm, ref, "film of the exact walk")
    assert_bit_equal(wfilm, ref, "film of the counting production walk")
    print({k: (cst[k], wk[k]) for k in COUNTERS})
    for k in COUNTERS:
        assert cst[k] == rst[k], (k, cst[k], rst[k])
    gold = json.load(open(GOLDEN))["mesh20k_64x64_2x2_depth8_seed3_host"]
    for k in COUNTERS:
        assert wk[k] == gold[k], (k, wk[k], gold[k])


@pytest.mark.gpu
@pytest.mark.parametrize("waves", ["1", "5"])
def test_mesh_film_from_few_persistent_waves(gpu, mesh, monkeypatch, waves):
    """1 and 5 persistent one-wave workgroups for the frame's 4 096 items: a wave's pixel list runs dry lane by lane, the lanes with work
    left (`alive`) shrink while others walk, and the exit test's walkers-wanted figure, taken once per call now, shrinks with them."""
    sd, ref, _ = mesh
    with gpu.Scene(sd, builder="host") as sc:
        monkeypatch.setenv("PBRT_HIP_RENDER_WORKGROUPS", waves)
        film, _ = sc.render(**MESH_KW)
    assert_bit_equal(film, ref, f"film from {waves} persistent wave(s)")


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["cornell", "sphere"])
def test_shallow_tree_films(gpu, oracle, name):
    """A 32 x 32 Cornell box at 2 x 2 spp: the whole stack in LDS, STEPS = 2, scalar plane fmas.  sphere_scene at 32 x 32: the SPH
    instantiation, whose leaf pass tests a sphere's record.  Films equal to the oracle's."""
    sd = scenes.cornell_scene(32, 32) if name == "cornell" else scenes.sphere_scene(32, 32)
    kw = dict(max_depth=5, spp=(2, 2), seed=1)
    ref, _ = oracle.OracleScene(sd).render(**kw)
    with gpu.Scene(sd) as sc:
        film, _ = sc.render(**kw)
    assert_bit_equal(film, ref, "film")


@pytest.mark.gpu
def test_ray_batches(gpu, oracle, mesh):
    """intersect_kernel shares trav_run: closest hits and occlusion flags of 10 000 rays through the mesh equal the oracle's, and the
    canonical counters (the EXACT walk of the batch kernel) too."""
    sd = mesh[0]
    o, d, tmax = random_rays(10_000 - 6, 17)
    assert len(o) == 10_000
    ref = oracle.OracleScene(sd)
    rt, rp, rb1, rb2, rc = ref.intersect(o, d, tmax)
    with gpu.Scene(sd, builder="host") as sc:
        t, prim, b1, b2, _ = sc.intersect(o, d, tmax)
        ct, cprim, _, _, cnt = sc.intersect(o, d, tmax, counters=True)
        occ = sc.occluded(o, d, tmax)
    assert (rp != 0xFFFFFFFF).mean() > 0.05
    for got, want, what in ((prim, rp, "prim"), (t, rt, "t"), (b1, rb1, "b1"), (b2, rb2, "b2"), (cprim, rp, "prim (exact walk)"), (ct, rt, "t (exact walk)")):
        assert_bit_equal(got, want, what)
    assert cnt == rc, (cnt, rc)
    assert_bit_equal(occ, ref.occluded(o, d, tmax), "occluded")
