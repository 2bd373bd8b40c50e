"""Writes scenes/sky_small.pfm, the 64 x 32 environment map of scenes/envmap_spheres.pbrt: pbrt_amd.scenes.procedural_sky(64, 32) through
the library's own PFM writer.  Host only; run from the repository root after building the library:

  python tools/make_sky_pfm.py [out.pfm [width height]]
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import pbrt_amd  # noqa: E402
from pbrt_amd import scenes  # noqa: E402

if __name__ == "__main__":
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(root, "scenes", "sky_small.pfm")
    w, h = (int(sys.argv[2]), int(sys.argv[3])) if len(sys.argv) > 3 else (64, 32)
    sky = scenes.procedural_sky(w, h)
    pbrt_amd.write_image(out, sky)
    back = pbrt_amd.read_image(out)
    assert back.shape == sky.shape and (back == sky).all(), "the PFM does not read back as written"
    print(f"{out}: {w} x {h}, max / mean radiance {sky.max() / sky.mean():.1f}")
