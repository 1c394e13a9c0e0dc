"""Tile moves scored by the objective, on one MI355X: synth_image() 256 x 256, 8 subpalettes x 15
colours, state after the k-means start + reassign_tiles.  Writes one JSON document (default profiles/tile_moves.json),
stamped with snesimage_version().

    python profiles/tile_moves.py [--parent-root DIR] [--out FILE] [--repeats 3]

Legs (each a child process of its own under a time limit; a failed child ends the run):
  score   candidates per second through score_tile_moves for lists of 7, 448 and 4,096 pairs, RGB and --dither, and
          score_candidates (palette candidates) at the same lengths for orientation;
  route   the same pairs through what a build without the feature offers: tile_palettes setter + optimize() + error() per
          pair.  With --parent-root this leg imports the package of that tree (a checkout of the parent commit, built), so
          the yardstick is the parent's own code; without it, this tree's.  score and route alternate, `--repeats` times;
  sweep   tile calls per second over full 1,024-tile sweeps, window 0 against window 1, first and third sweep;
  buys    the error after k-means, reassign_tiles, one and three tile sweeps, and 3 x 120 scheduled palette calls with a
          tile sweep / reassign_tiles / nothing after every 120."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LENGTHS = (7, 448, 4096)
COUNT, SIZE = 8, 15


def start(root, dither, reassign=True):
    sys.path.insert(0, root)
    import numpy as np
    import snesimage_amd as S
    from snesimage_amd.synth import synth_image
    g = S.OptimizedImage(synth_image(), COUNT, SIZE, dither=dither)
    g.initialize_tiles()
    g.recalculate_palettes()
    e0 = g.error()
    if reassign:
        g.reassign_tiles()
    return S, np, g, e0


def pairs_for(np, g, n):
    rng = np.random.default_rng(n)
    tiles = rng.integers(0, 1024, n)
    tp = g.tile_palettes
    subs = (tp[tiles] + 1 + rng.integers(0, COUNT - 1, n)) % COUNT  # never the tile's own subpalette
    return tiles.astype(np.uint16), subs.astype(np.uint8)


def timed(fn, min_s=1.0, min_reps=2):
    fn()  # warm-up for this shape
    reps, t0 = 0, time.perf_counter()
    while True:
        fn()
        reps += 1
        dt = time.perf_counter() - t0
        if reps >= min_reps and dt >= min_s:
            return dt / reps


def child_score(root, dither):
    S, np, g, _ = start(root, dither)
    from snesimage_amd import _ffi
    out = {"leg": "score", "dither": dither, "build": _ffi.load().snesimage_version().decode(), "rates": {}, "palette_rates": {}}
    for n in LENGTHS:
        tiles, subs = pairs_for(np, g, n)
        out["rates"][str(n)] = round(n / timed(lambda: g.score_tile_moves(tiles, subs)), 1)
        cand = S.random_candidates(1, n, n)
        out["palette_rates"][str(n)] = round(n / timed(lambda: g.score_candidates(3, 5, cand)), 1)
    print(json.dumps(out))


def child_route(root, dither):
    S, np, g, _ = start(root, dither)
    from snesimage_amd import _ffi
    out = {"leg": "route", "dither": dither, "build": _ffi.load().snesimage_version().decode(), "rates": {}}
    tp0 = g.tile_palettes

    def route(tiles, subs):
        for t, k in zip(tiles, subs):
            tp = tp0.copy()
            tp[t] = k
            g.tile_palettes = tp
            g.optimize()
            g.error()
    for n in LENGTHS:
        tiles, subs = pairs_for(np, g, n)
        route(tiles[:7], subs[:7])
        t0 = time.perf_counter()
        route(tiles, subs)
        out["rates"][str(n)] = round(n / (time.perf_counter() - t0), 1)
    print(json.dumps(out))


def child_sweep(root, dither):
    out = {"leg": "sweep", "dither": dither, "windows": {}}
    for window in (0, 1):
        S, np, g, _ = start(root, dither)
        g.score_tile_moves(*pairs_for(np, g, 512))  # allocates the workspace of a full launch group: not what is timed
        rows = []
        for sweep in range(3):
            t0 = time.perf_counter()
            log, st = g.tile_sweep(0, 1024, window)
            dt = time.perf_counter() - t0
            rows.append({"sweep": sweep + 1, "calls_per_s": round(1024 / dt, 1), "accepted": st["accepted"], "launch_sets": st["windows"],
                         "scored_per_useful": round(st["scored"] / st["useful"], 3), "error": float(log["error"][-1])})
        out["windows"][str(window)] = rows
        g.close()
    print(json.dumps(out))


def child_buys(root, dither):
    out = {"leg": "buys", "dither": dither}
    S, np, g, e0 = start(root, dither, reassign=False)
    out["error_kmeans"] = e0
    g.reassign_tiles()
    out["error_reassign"] = g.error()
    errs = []
    for _ in range(3):
        log, _ = g.tile_sweep()
        errs.append(g.error())
    out["error_sweep1"], out["error_sweep3"] = errs[0], errs[2]
    g.close()
    for mode in ("none", "tile_moves", "reassign_tiles"):
        S, np, g, _ = start(root, dither, reassign=False)
        st = (0, 0, 0, 0)
        for r in range(3):
            _, st, _ = g.run_slots(120, seed=1, first_step_id=120 * r, state=st, want_log=False)
            if mode == "tile_moves":
                g.tile_sweep()
            elif mode == "reassign_tiles":
                g.reassign_tiles()
        out["run_360_" + mode] = g.error()
        g.close()
    print(json.dumps(out))


CHILDREN = {"score": child_score, "route": child_route, "sweep": child_sweep, "buys": child_buys}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-root", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tile_moves.json"))
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--timeout", type=int, default=300)
    ap.add_argument("--legs", default="score,sweep,buys")
    ap.add_argument("--child", nargs=3, metavar=("LEG", "ROOT", "DITHER"))
    a = ap.parse_args()
    if a.child:
        CHILDREN[a.child[0]](a.child[1], a.child[2] == "1")
        return 0

    def run(leg, root, dither):
        cmd = [sys.executable, os.path.abspath(__file__), "--child", leg, root, "1" if dither else "0"]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.timeout, cwd=root)
        if r.returncode != 0:
            raise RuntimeError("%s leg failed (rc %d): %s" % (leg, r.returncode, r.stderr[-600:]))  # nothing more is started on the device
        return json.loads(r.stdout.strip().splitlines()[-1])

    legs = a.legs.split(",")
    doc = {"image": "synth_image() 256x256", "geometry": [COUNT, SIZE], "route_root": "parent" if a.parent_root else "this tree", "score": [], "sweep": [], "buys": []}
    if "score" in legs:
        for dither in (False, True):
            runs = {"score": [], "route": []}
            for _ in range(a.repeats):  # the two sides alternate
                runs["score"].append(run("score", ROOT, dither))
                runs["route"].append(run("route", a.parent_root or ROOT, dither))
            doc["build"] = runs["score"][0]["build"]
            doc["route_build"] = runs["route"][0]["build"]
            for n in LENGTHS:
                s = [r["rates"][str(n)] for r in runs["score"]]
                p = [r["rates"][str(n)] for r in runs["route"]]
                c = [r["palette_rates"][str(n)] for r in runs["score"]]
                doc["score"].append({"dither": dither, "pairs": n, "tile_moves_per_s": statistics.median(s), "tile_moves_spread": [min(s), max(s)],
                                     "route_per_s": statistics.median(p), "route_spread": [min(p), max(p)], "ratio": round(statistics.median(s) / statistics.median(p), 2),
                                     "worst_ratio": round(min(s) / max(p), 2), "palette_candidates_per_s": statistics.median(c)})
                print(json.dumps(doc["score"][-1]), flush=True)
    for leg in ("sweep", "buys"):
        if leg in legs:
            for dither in (False, True):
                doc[leg].append(run(leg, ROOT, dither))
                print(json.dumps(doc[leg][-1]), flush=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
