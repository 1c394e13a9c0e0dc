"""What a native export costs next to as_tilemap_json: 256 x 224, 8 x 15, a host clock around calls that end in a device
synchronise (the Python methods: export_native is the sizes-only call and the full call).  python profiles/native_export.py [--out FILE]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

import snesimage_amd as S
from snesimage_amd import _ffi
from snesimage_amd.synth import synth_image

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "native_export.json"))
args = ap.parse_args()

img = synth_image(0x5EED0000, 256, 224)
g = S.OptimizedImage(img, 8, 15)
g.initialize_tiles()
g.recalculate_palettes()


def timed(fn, n=50, warm=5):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(n):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    ts = np.array(ts)
    return dict(median_ms=float(np.median(ts)), min_ms=float(ts.min()), max_ms=float(ts.max()), n=n)


ex = g.export_native()
out = dict(library=_ffi.load().snesimage_version().decode(), shape="256x224 8x15", unique=ex["unique"], bpp=ex["bpp"],
           characters=timed(g.characters), as_tilemap_json=timed(g.as_tilemap_json), export_native=timed(g.export_native),
           render_native=timed(lambda: g.render_native(ex["cgram"], ex["chr"], ex["map"], bpp=ex["bpp"])), as_rgba=timed(g.as_rgba))
print(json.dumps(out))
json.dump(out, open(args.out, "w"), indent=1)
