"""What palette blocks (snesimage_set_palette_blocks, DESIGN 4b'') cost: the bench image cut to 256 x 224 (896 tiles), 8 x 15, RGB,
one MI355X, for blocks of 1 x 1, 2 x 2 and 4 x 4 tiles.  An observation: no threshold, no speed claim.

    python profiles/blocks.py [--calls 120] [--repeats R] [--parent DIR] [--out profiles/blocks.json]

Every leg starts from the initialisers at its granularity, runs `--calls` calls of the reference's loop through
snesimage_run_slots (120 = one sweep of the 8 x 15 palette: the schedule of `--tile-moves 1`), and then sweeps all blocks once
with snesimage_block_sweep, from the same state with window 0 (sized by the library) and window 1 (call by call): the wall time
of the sweep per block call and per candidate scored, the calls accepted, and error() in front of and behind the sweep.  The
1 x 1 leg also times snesimage_tile_sweep, which must do the same work.  --parent DIR: a checkout of the parent commit (its
library built): its snesimage_tile_sweep runs from it on the same box, the legs alternating.
Every measurement is a child process of its own under a time limit; a child that fails ends the run: nothing more is started
on the device.  The output is stamped with the library's source hash."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BLOCKS = ((1, 1), (2, 2), (4, 4))


def child(a):
    sys.path.insert(0, a.root)
    import numpy as np
    import snesimage_amd as S
    from snesimage_amd import _ffi
    from snesimage_amd.synth import synth_image
    img = np.ascontiguousarray(synth_image(0x5EED0000)[:224])
    bw, bh = (int(v) for v in a.blocks.split("x"))
    parent = a.leg == "parent_tile"
    g = S.OptimizedImage(img, 8, 15)
    if not parent:
        g.palette_blocks = (bw, bh)
    g.initialize_tiles()
    g.recalculate_palettes()
    g.run_slots(a.calls, seed=1, first_step_id=0, want_log=False)
    tp, pal = g.tile_palettes, g.palette
    out = {"leg": a.leg, "blocks": a.blocks, "version": _ffi.load().snesimage_version().decode(), "calls": a.calls, "error_before": g.error(), "sweeps": []}
    sweeps = [("tile_sweep", g.tile_sweep)] if parent else [("block_sweep", g.block_sweep)] + ([("tile_sweep", g.tile_sweep)] if bw * bh == 1 else [])
    for name, sweep in sweeps:
        for window in (0, 0, 1):  # the first one allocates the workspace and is not reported
            g.tile_palettes, g.palette = tp, pal
            g.optimize()
            g.error()
            g.sync()
            t0 = time.perf_counter()
            log, stats = sweep(0, None, window)
            ms = 1e3 * (time.perf_counter() - t0)
            rec = {"call": name, "window": window, "ms": ms, "ms_per_call": ms / len(log), "ms_per_candidate": ms / max(1, stats["scored"]), "calls": len(log),
                   "accepted": stats["accepted"], "windows": stats["windows"], "scored": stats["scored"], "error_after": g.error()}
            out["sweeps"].append(rec)
        out["sweeps"].pop(-3)
    print(json.dumps(out))
    return 0


def run_child(a, root, leg, blocks):
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--leg", leg, "--root", root, "--calls", str(a.calls), "--blocks", blocks]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.timeout)
    if r.returncode != 0:
        print(json.dumps({"failed": cmd[2:], "rc": r.returncode, "stderr": r.stderr[-600:]}), flush=True)
        sys.exit(1)
    return json.loads(r.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=120)
    ap.add_argument("--repeats", type=int, default=2)
    ap.add_argument("--parent", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "blocks.json"))
    ap.add_argument("--timeout", type=int, default=240)
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--leg", choices=["blocks", "parent_tile"], default="blocks")
    ap.add_argument("--blocks", default="1x1")
    ap.add_argument("--root", default=ROOT)
    a = ap.parse_args()
    if a.child:
        return child(a)
    res = {"runs": []}
    for _ in range(a.repeats):  # the legs alternate
        legs = [("blocks", ROOT, "%dx%d" % b) for b in BLOCKS] + ([("parent_tile", os.path.abspath(a.parent), "1x1")] if a.parent else [])
        for leg, root, blocks in legs:
            r = run_child(a, root, leg, blocks)
            res["runs"].append(r)
            print(json.dumps(r), flush=True)
    res["library"] = next(r["version"] for r in res["runs"] if r["leg"] == "blocks")
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
