"""Random scenes with substrate materials for tests/test_substrate_gpu.py, from a seed space of their own
(np.random.default_rng(124_000 + seed)): a small random mesh with a few spheres under random lights, materials matte / mirror / emissive
as tests/util.py's random_scene draws them, and then EVERY THIRD matte primitive (triangles and spheres counted together, in order) moved to
one of five substrate materials: alpha 1e-3, 0.05, 0.3 with Ks = 0, 1, and 0.3 with Kd = 0.  No texture, no map, no normals, whole images, and
no sphere smaller than 0.15 (a grazing hit on a tiny sphere is float32's sphere discriminant, not this material)."""
import numpy as np

from pbrt_amd import MATTE, MIRROR, SUBSTRATE, SceneData, look_at

N_SEEDS = 12
ALPHAS = (1e-3, 0.05, 0.3, 1.0, 0.3)


def random_substrate_case(seed):
    """-> (scene, render arguments) number `seed`"""
    rng = np.random.default_rng(124_000 + seed)
    n_tris = int(rng.choice([5, 17, 64, 200]))
    c = rng.uniform(-1, 1, (n_tris, 1, 3))
    P = (c + rng.uniform(-0.5, 0.5, (n_tris, 3, 3))).reshape(-1, 3).astype(np.float32)
    idx = np.arange(3 * n_tris, dtype=np.uint32).reshape(-1, 3)
    n_base = int(rng.integers(2, 6))
    mats = []
    for m in range(n_base):
        kind = MIRROR if (m > 0 and rng.random() < 0.25) else MATTE
        le = tuple(rng.uniform(0.5, 8.0, 3)) if (kind == MATTE and m > 0 and rng.random() < 0.3) else (0, 0, 0)
        mats.append([kind, *rng.uniform(0.1, 0.95, 3), *le])
    mat_id = rng.integers(0, n_base, n_tris).astype(np.int64)
    spheres = np.array([[*rng.uniform(-1, 1, 3), rng.uniform(0.15, 0.6), int(rng.integers(0, n_base))] for _ in range(int(rng.integers(0, 3)))]).reshape(-1, 5)
    # the five substrate materials, appended; every third plain matte primitive moves to them in turn
    for j, alpha in enumerate(ALPHAS):
        kd, ks = rng.uniform(0.1, 0.9, 3), rng.uniform(0.05, 0.9, 3)
        if j == 2:
            ks = np.zeros(3)
        if j == 4:
            kd = np.zeros(3)
        mats.append([SUBSTRATE, *kd, *ks])
    mats = np.array(mats, np.float32)
    beside = np.concatenate([np.full(n_base, 1.5), ALPHAS]).astype(np.float32)
    plain = (mats[:n_base, 0] == MATTE) & ~(mats[:n_base, 4:7] > 0).any(1)
    count = 0
    for t in range(n_tris):
        if plain[mat_id[t]]:
            if count % 3 == 0:
                mat_id[t] = n_base + (count // 3) % 5
            count += 1
    for s in range(len(spheres)):
        if plain[int(spheres[s, 4])]:
            if count % 3 == 0:
                spheres[s, 4] = n_base + (count // 3) % 5
            count += 1
    lights = []
    for _ in range(int(rng.integers(1, 4))):
        kind = int(rng.integers(0, 3))
        if kind == 2:
            lights.append([kind, 0, 0, 0, *rng.uniform(0.1, 1.0, 3)])
        elif kind == 1:
            d = rng.normal(size=3)
            lights.append([kind, *(d / np.linalg.norm(d)), *rng.uniform(0.5, 3.0, 3)])
        else:
            lights.append([kind, *rng.uniform(-3, 3, 3), *rng.uniform(2.0, 30.0, 3)])
    eye = rng.uniform(-3.5, 3.5, 3)
    if np.linalg.norm(eye) < 1.5:
        eye = eye / max(np.linalg.norm(eye), 1e-3) * 2.5
    sd = SceneData(P=P, idx=idx, mat_id=mat_id.astype(np.uint16), materials=mats, mat_eta=beside, lights=np.array(lights, np.float32).reshape(-1, 7),
                   spheres=spheres.astype(np.float32), cam_to_world=look_at(tuple(eye), tuple(rng.uniform(-0.3, 0.3, 3)), (0, 0, 1))[1],
                   fov=float(rng.uniform(25, 100)), xres=int(rng.integers(8, 40)), yres=int(rng.integers(8, 40))).normalized()
    kw = dict(integrator=(0, 1, 2)[seed % 3], max_depth=int(rng.integers(1, 8)), spp=(int(rng.integers(1, 4)), int(rng.integers(1, 4))),
              seed=int(rng.integers(0, 1 << 20)), sampler=("stratified", "sobol", "halton", "sobol_nd")[(seed // 3) % 4])
    if seed % 4 == 1:
        kw["filter_width"] = (float(rng.choice([1.0, 1.5, 2.5])), float(rng.choice([0.75, 1.0, 2.0])))
    if seed % 4 == 2:
        kw["max_sample_luminance"] = float(rng.choice([0.25, 1.0, 4.0]))
    return sd, kw
