"""DESIGN.md section 6.25, the CPU-side count: how many pixels of a scene's frame end at bounce 0 with colour 0 (the first-state
table's kind FS_ZERO), with a constant colour (FS_CONST) or survive, and how many 64-pixel camera tiles consist of FS_ZERO pixels
only -- from the oracle alone, no device.  Survivors: the pool after bounce 0 of one iteration at depth 2; a constant colour: a
pixel that is not zero after one iteration at depth 1 (bounce 0 is then the last bounce: only emitters score).
    python profiles/first_state/count_ended.py [SCENE.txt]"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402
from oracle import pyoracle as po  # noqa: E402


def main(path):
    pt = ge.load_package()
    scn = pt.load_scene(path)
    w, h = scn.resolution
    n = w * h
    geoms = scn.geoms.view(po.GEOM_DT)
    snaps = []
    po.Tracer(geoms, scn.materials, scn.camera, 2, flags=po.F_COMPACT, trig=po.TRIG_SHARED).iterate(1, snapshots=snaps)
    live = np.zeros(n, dtype=bool)
    live[snaps[0]["paths"]["pixelIndex"][:snaps[0]["n_live"]]] = True
    one = po.Tracer(geoms, scn.materials, scn.camera, 1, flags=po.F_COMPACT, trig=po.TRIG_SHARED)
    one.iterate(1)
    const = (np.asarray(one.image).reshape(n, 3) != 0).any(axis=1) & ~live
    zero = ~live & ~const
    tiles = n // 64
    whole = zero[:tiles * 64].reshape(tiles, 64).all(axis=1)
    out = {"scene": os.path.relpath(path, ROOT), "frame": [w, h], "pixels": n, "survive_bounce_0": int(live.sum()),
           "end_with_constant_colour": int(const.sum()), "end_with_colour_0": int(zero.sum()),
           "end_with_colour_0_share": float(zero.sum()) / n, "tiles_of_64": tiles, "tiles_all_colour_0": int(whole.sum()),
           "tiles_all_colour_0_share": float(whole.sum()) / tiles, "pixels_no_multiple_of_64": n % 64 != 0}
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "scenes", "cornell.txt"))
