"""What a native import costs next to the four setters done by hand: 256 x 224, 8 x 15, a host clock around calls that end in a
device synchronise (the Python methods).  The bytes are the image's own export; the hand-made state is what the test model would
parse from them, read from the context itself.  python profiles/native_import.py [--out FILE]"""
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
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "native_import.json"))
args = ap.parse_args()

img = synth_image(0x5EED0000, 256, 224)
g = S.OptimizedImage(img, 8, 15)
g.initialize_tiles()
g.recalculate_palettes()
ex = g.export_native()
pal, tp, pm = g.palette, g.tile_palettes, g.palette_map
x = S.OptimizedImage(img, 8, 15)


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


def setters():
    x.palette = pal
    x.tile_palettes = tp
    x.palette_map = pm


out = dict(library=_ffi.load().snesimage_version().decode(), shape="256x224 8x15", unique=ex["unique"], bpp=ex["bpp"],
           import_native=timed(lambda: x.import_native(ex["cgram"], ex["chr"], ex["map"])), three_setters=timed(setters),
           export_native=timed(g.export_native))
assert np.array_equal(x.palette_map, pm) and np.array_equal(x.palette, pal)
print(json.dumps(out))
json.dump(out, open(args.out, "w"), indent=1)
