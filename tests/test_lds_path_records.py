"""Path records 0..2 in LDS behind a shorter walk stack (device_types.h kLdsPathRecords, kernel_path.hpp path_load / path_store): the default
path's overflow instantiation keeps {L, flags}{beta, rng lo}{wi_next, rng hi} of every lane in three 1 KB rows behind 18 stack rows instead of
in HBM.  Nothing computed changes: films equal the oracle's bit for bit, the walk does the same work, a walk deeper than the 18 rows goes to the
HBM overflow area and not into the record rows, and a lane that takes a new item leaves its neighbours' records alone."""
import ctypes as C
import dataclasses
import json
import os

import numpy as np
import pytest

from pbrt_amd import LIGHT_INFINITE, MATTE, SceneData, _lib, look_at, scenes
from util import assert_bit_equal

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lds_path_records_walk.json")
COUNTERS = ("camera_rays", "bounce_rays", "shadow_rays", "nodes_visited", "tris_tested")


def layout(need):
    rows, rec, waves, extra = C.c_uint32(), C.c_uint32(), C.c_uint32(), C.c_uint32()
    assert _lib.lib().pbrt_hip_render_stack_layout(need, C.byref(rows), C.byref(rec), C.byref(waves), C.byref(extra)) == 0
    return rows.value, rec.value, waves.value, extra.value


def test_plan_arithmetic():
    """pbrt_hip_render_stack_layout, the default path's launch: a tree whose stack fits 30 rows keeps it whole in LDS and its records in HBM; a
    deeper one gets 18 stack rows and 3 KB of records -- the same 7 680 bytes, six granules, 20 waves per CU -- and need + 2 - 18 entries
    per lane in HBM.  (pbrt_hip_render_stack_plan stays the plan of every other launch: 30 rows, tests/test_host.py.)"""
    for need in (6, 16, 17, 28, 29, 44, 48):
        rows, rec, waves, extra = layout(need)
        assert rows * 256 + rec <= 7680 and waves == 20, (need, rows, rec, waves)
        assert extra == max(0, need + 2 - rows) and (extra == 0 or rows + extra == need + 2), (need, rows, extra)
        if need <= 28:
            assert (rows, rec, extra) == (max(8, need + 2), 0, 0), (need, rows, rec, extra)
        else:
            assert (rows, rec) == (18, 3072) and rows * 256 + rec == 7680, (need, rows, rec)
            old = tuple(C.c_uint32() for _ in range(3))
            assert _lib.lib().pbrt_hip_render_stack_plan(need, *map(C.byref, old)) == 0
            assert (old[0].value, old[1].value, old[2].value) == (30, 20, need + 2 - 30)  # what the variants' kernels (STACK = 30) keep


LLVM = "/opt/rocm/lib/llvm/bin"


@pytest.mark.skipif(not os.path.exists(os.path.join(LLVM, "llvm-objdump")), reason="needs the ROCm llvm tools")
def test_records_are_single_b128_accesses_behind_the_stack():
    """kernel_path.hpp states a record as four scalar accesses of a 16-byte-aligned struct and leaves the joining to the compiler.  This pins
    what it must come out as in the production instantiation: per service visit three ds_read_b128 and three ds_write_b128 whose immediate
    offsets are the records' places, 18 x 256 + k x 1024 -- inside the launch's 7 680 bytes, behind the walk's 18 rows -- and no narrower LDS
    access at those places."""
    import glob
    import re
    import shutil
    import subprocess
    import tempfile
    sym = "_ZN8pbrt_hip12_GLOBAL__N_113render_kernelILb0ELb0ELb0ELi30ELi3ELb0ELb0EEEvNS_8DevSceneENS_12RenderParamsE"
    with tempfile.TemporaryDirectory() as td:
        so = shutil.copy(_lib.LIB_PATH, td)
        subprocess.run([os.path.join(LLVM, "llvm-objdump"), "--offloading", os.path.basename(so)], cwd=td, check=True, capture_output=True)
        text = ""
        for co in sorted(glob.glob(os.path.join(td, "*gfx950"))):
            r = subprocess.run([os.path.join(LLVM, "llvm-objdump"), "-d", "--disassemble-symbols=" + sym, co], capture_output=True, text=True)
            if "ds_" in r.stdout:
                text = r.stdout
    assert text, "the production instantiation was not found in the library's gfx950 code objects"
    places = [18 * 256 + k * 1024 for k in range(3)]
    for op in ("ds_read_b128", "ds_write_b128"):
        got = sorted(int(m) for m in re.findall(op + r"\s[^\n]*offset:(\d+)", text))
        assert got == places, (op, got)
    others = [m for m in re.findall(r"(ds_\w+)\s[^\n]*offset:(\d+)", text) if int(m[1]) >= places[0] and not m[0].endswith("_b128")]
    assert not others, others


def stacked_sliver_scene(k=400, res=64):
    """k large triangles facing the camera, stacked behind each other at distances that shrink geometrically (the SAH peels a few off per
    level: a deep tree) and growing in size: a camera ray descends to the NEAREST layer first, through every level of the tree, and stacks the
    siblings it will visit later -- more of them the nearer it is to the middle of the image"""
    i = np.arange(k)
    z = (0.5 ** (i / 2.0)).astype(np.float32)
    s = (0.2 + 0.8 * i / k).astype(np.float32)
    P = np.concatenate([np.stack([-s, -s, z], 1), np.stack([s, -s, z], 1), np.stack([0 * s, s, z], 1)]).astype(np.float32)
    idx = np.stack([i, k + i, 2 * k + i], 1).astype(np.uint32)
    return SceneData(P=P, idx=idx, mat_id=(i % 2).astype(np.uint16), materials=np.array([[MATTE, .6, .5, .4, 0, 0, 0], [MATTE, .3, .7, .5, 0, 0, 0]], np.float32),
                     lights=np.array([[LIGHT_INFINITE, 0, 0, 0, 1, 1, 1]], np.float32),
                     cam_to_world=look_at((0.0, -0.2, -2.0), (0, -0.2, 0), (0, 1, 0))[1], fov=50, xres=res, yres=res).normalized()


def deepest_stacks(oracle, sd, quads, order, monkeypatch):
    """the deepest stack of every pixel-centre camera ray's walk through the tree as it sits in HBM (oracle/quad_walk.cpp, the kernel's
    step restated; tools/walk_sim.py's stack-depth output: ORC_WALK_STACK_IN_TRIS puts it into the high half of the triangle count)"""
    monkeypatch.setenv("ORC_WALK_STACK_IN_TRIS", "1")
    osc = oracle.OracleScene(sd)
    rays = [osc.camera_ray(x + 0.5, y + 0.5) for y in range(sd.yres) for x in range(sd.xres)]
    o, d = np.array([r[0] for r in rays], np.float32), np.array([r[1] for r in rays], np.float32)
    V = sd.P.reshape(-1, 3)[sd.idx.reshape(-1)]
    c = oracle.quad_walk(quads, np.concatenate([V.min(0), V.max(0)]), sd.P, sd.idx, order, o, d, np.full(len(o), np.inf, np.float32))
    return c["tris"] >> 16


@pytest.mark.gpu
def test_film_and_walk_counters(gpu, oracle):
    """20 000 random triangles on the host builder's tree (stack bound 29: the overflow variant), 64 x 64 at 2 x 2 spp, depth 8, stratified:
    the film -- rendered by the instantiation with the records in LDS -- is the oracle's.  The walk counters come from the COUNTING
    instantiation, which keeps its records in HBM and its 30 rows (render_variant.hpp render_default_path): comparing them with the totals
    recorded before the records moved (tests/golden/) checks that the counting kernel and the tree were left alone, not the new path -- the
    film assertion is what covers that here."""
    sd = scenes.random_mesh_scene(20_000, 64, 64)
    kw = dict(max_depth=8, spp=(2, 2), seed=3)
    ref, _ = oracle.OracleScene(sd).render(**kw)
    with gpu.Scene(sd, builder="host") as sc:
        need = sc.info()["quad_stack_need"]
        rows, rec, waves, extra = layout(need)
        assert rec == 3072 and rows == 18 and extra == need + 2 - 18, (need, rows, rec, extra)  # the precondition: records in LDS
        film, _ = sc.render(**kw)
        _, wk = sc.render(counters="walk", **kw)
    assert_bit_equal(film, ref, "film")
    gold = json.load(open(GOLDEN))["mesh20k_64x64_2x2_depth8_seed3_host"]
    print({k: wk[k] for k in COUNTERS})
    for k in COUNTERS:
        assert wk[k] == gold[k], (k, wk[k], gold[k])


@pytest.mark.gpu
def test_deep_walks_reach_the_hbm_overflow_behind_the_records(gpu, oracle, monkeypatch):
    """400 stacked slivers: hundreds of camera rays hold more than the 16 entries that 18 rows keep (sentinel and scratch row aside), up to 19, so
    their pushes go past the LDS part -- into the HBM overflow area, not into the record rows that follow the stack: film equal to the oracle's."""
    sd = stacked_sliver_scene()
    kw = dict(max_depth=8, spp=(2, 2), seed=1)
    ref, _ = oracle.OracleScene(sd).render(**kw)
    with gpu.Scene(sd, builder="host") as sc:
        rows, rec, _, extra = layout(sc.info()["quad_stack_need"])
        assert rec == 3072 and extra > 0
        quads, order = sc.export_quads()
        film, _ = sc.render(**kw)
    depth = deepest_stacks(oracle, sd, quads, order, monkeypatch)
    print("deepest stack per camera ray:", np.bincount(depth))
    assert (depth > rows - 2).sum() >= 100 and (depth == rows - 2).any() and (depth == rows - 3).any(), np.bincount(depth)
    assert_bit_equal(film, ref, "film")


@pytest.mark.gpu
def test_item_hand_over_keeps_the_neighbours_records(gpu, oracle, monkeypatch):
    """A lane that finishes its item draws the next one while its neighbours' path state stays parked in the same three LDS rows.  That needs
    fewer lanes than items: the launch is cut to 2 and to 5 persistent one-wave workgroups (PBRT_HIP_RENDER_WORKGROUPS, as
    test_gpu_parity.py::test_item_handout_is_scheduling_only does on a shallow tree, whose kernels keep their records in HBM), on the mesh
    scene that takes the overflow variant.  64 spp on a 16 x 16 crop: 512 items of 32 samples in runs of 64 among the super-tile's 8 192
    slots, 128 or 320 lanes; a wave's lanes finish at different times and every later draw refills a few of them beside parked neighbours.
    The whole 64 x 64 frame at 2 x 2 spp on 5 waves: 4 096 items, 13 in turn per lane.  Films equal to the oracle's.  (With the default
    grid a frame of this size has a lane per item slot and no lane ever draws twice.)"""
    mesh = scenes.random_mesh_scene(20_000, 64, 64)
    sd = dataclasses.replace(mesh, crop=(0.375, 0.625, 0.375, 0.625)).normalized()
    assert sd.crop_size() == (16, 16)
    kw, kw_whole = dict(max_depth=8, spp=(8, 8), seed=7), dict(max_depth=8, spp=(2, 2), seed=3)
    ref, _ = oracle.OracleScene(sd).render(**kw)
    ref_whole, _ = oracle.OracleScene(mesh).render(**kw_whole)
    films = {}
    with gpu.Scene(sd, builder="host") as sc:
        assert layout(sc.info()["quad_stack_need"])[1] == 3072
        for n in ("2", "5"):
            monkeypatch.setenv("PBRT_HIP_RENDER_WORKGROUPS", n)
            films[n] = sc.render(**kw)[0]
    with gpu.Scene(mesh, builder="host") as sc:
        monkeypatch.setenv("PBRT_HIP_RENDER_WORKGROUPS", "5")
        whole = sc.render(**kw_whole)[0]
    for n, film in films.items():
        assert_bit_equal(film, ref, f"film of the crop from {n} persistent waves")
    assert_bit_equal(whole, ref_whole, "film of the whole frame from 5 persistent waves")
