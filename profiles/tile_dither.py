"""What per-tile ordered-dither levels (snesimage_level_sweep, DESIGN 5d') cost and gain: the bench image (256 x 256, 8 x 15,
RGB, Bayer 4 x 4 at amplitude 32), one MI355X.

    python profiles/tile_dither.py [--calls 2400] [--levels 4] [--repeats R] [--out profiles/tile_dither.json]

Legs, every one a child process of its own under a time limit (a child that fails ends the run: nothing more is started on the
device):
  sweep   from the k-means initialisers and 240 calls of the reference's loop: one level sweep over all 1,024 tiles
          (snesimage_level_sweep, window 0), timed by the host clock around the synchronous call after an untimed sweep over
          the first 64 tiles has sized the workspace -> candidates per second, calls per second, launch sets, accepted; then,
          in the same process and state, a tile sweep (snesimage_tile_sweep, window 0) over all tiles timed the same way.
          Both go through the same dense scorer with one palette_map per candidate: a large gap in candidates per second
          points at k_level_remap / k_level_commit, not at the scorer;
  plain   `--calls` calls of the reference's loop with the plain table (--ordered-dither 4) -> error();
  levels  the same number of optimizer calls with a level sweep behind every sweep of the palette and one behind the last call
          (--tile-dither 1 --dither-levels L) -> error().
The output is stamped with the library's source hash."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def ladder(S, n, amp, L):
    import numpy as np
    return np.stack([np.zeros((n, n), np.int8)] + [S.bayer_offsets(n, amp * j // (L - 1)) for j in range(1, L)])


def child(a):
    sys.path.insert(0, ROOT)
    import snesimage_amd as S
    from snesimage_amd import _ffi
    from snesimage_amd.synth import synth_image
    g = S.OptimizedImage(synth_image(0x5EED0000), 8, 15)
    if a.leg == "plain":
        g.set_ordered_dither(S.bayer_offsets(4, a.amplitude))
    else:
        g.set_ordered_dither_bank(ladder(S, 4, a.amplitude, a.levels), a.levels - 1)
    g.initialize_tiles()
    g.recalculate_palettes()
    out = {"leg": a.leg, "version": _ffi.load().snesimage_version().decode(), "error_start": g.error(), "levels": a.levels}
    if a.leg == "sweep":
        g.run_slots(240, seed=1, want_log=False)
        g.level_sweep(0, 64)  # sizes the workspace
        g.sync()
        e0 = g.error()
        t0 = time.perf_counter()
        _, st = g.level_sweep()
        dt = time.perf_counter() - t0
        out.update(level_sweep_s=dt, level_candidates_per_s=st["scored"] / dt, level_calls_per_s=st["calls"] / dt, level_windows=st["windows"], level_accepted=st["accepted"],
                   error_before=e0, error_after=g.error())
        g.tile_sweep(0, 64)
        g.sync()
        t0 = time.perf_counter()
        _, st = g.tile_sweep()
        dt = time.perf_counter() - t0
        out.update(tile_sweep_s=dt, tile_candidates_per_s=st["scored"] / dt, tile_calls_per_s=st["calls"] / dt, tile_windows=st["windows"], tile_accepted=st["accepted"])
    else:  # the CLI's loop: a level sweep behind every sweep of the palette and one behind the last call
        state, done, sweeps, accepted = (0, 0, 0, 0), 0, 0, 0
        per_sweep = next(k for k, r in enumerate(S.schedule(8, 15, 8 * 15 * 3 + 2)) if r[4] != 0)
        while done < a.calls:
            n = min(per_sweep - done % per_sweep, a.calls - done)
            _, state, _ = g.run_slots(n, seed=1, first_step_id=done, state=state, want_log=False)
            done += n
            if a.leg == "levels" and done % per_sweep == 0:
                accepted += g.level_sweep()[1]["accepted"]
                sweeps += 1
        if a.leg == "levels":
            accepted += g.level_sweep()[1]["accepted"]
            sweeps += 1
        out.update(calls=a.calls, error=g.error(), level_sweeps=sweeps, level_accepted=accepted)
        if a.leg == "levels":
            lv = g.tile_levels
            out["tiles_per_level"] = [int((lv == l).sum()) for l in range(a.levels)]
    print(json.dumps(out))
    return 0


def run_child(a, leg):
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--leg", leg, "--calls", str(a.calls), "--levels", str(a.levels), "--amplitude", str(a.amplitude)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.timeout)
    if r.returncode != 0:
        print(json.dumps({"failed": cmd[2:], "rc": r.returncode, "stderr": r.stderr[-600:]}), flush=True)
        sys.exit(1)
    return json.loads(r.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=2400)
    ap.add_argument("--levels", type=int, default=4)
    ap.add_argument("--amplitude", type=int, default=32)
    ap.add_argument("--repeats", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tile_dither.json"))
    ap.add_argument("--timeout", type=int, default=240)
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--leg", choices=["sweep", "plain", "levels"], default="sweep")
    a = ap.parse_args()
    if a.child:
        return child(a)
    res = {"runs": []}
    for _ in range(a.repeats):
        for leg in ("sweep", "plain", "levels"):
            r = run_child(a, leg)
            res["runs"].append(r)
            print(json.dumps(r), flush=True)
    res["library"] = res["runs"][0]["version"]
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
